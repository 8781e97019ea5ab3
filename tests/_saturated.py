"""Inputs of a trained agent for the head, draw and LSTM kernels, and the CPU side of their checks.

Test infrastructure only (imported by tests/test_saturated_cpu.py and
tests/test_gpu_saturated_heads.py).  Every other test feeds the kernels the logits of a freshly
initialised net (top-two gap 1 to 2, targets N(0, 1), LSTM biases 0.1 N(0, 1)).  A trained policy is
close to deterministic, its logits carry a common offset, its values reach hundreds and its LSTM
gates sit at 0 or 1.  There the kernels rest on the max-shift in front of every expf, on expf
underflowing to exactly 0, on pi log pi at pi = 0, on the cancellation in 1 - pi(a), on
1 / (1 + expf(-x)) with expf = inf, and on tanhf = +-1.

Rule for every tolerance: a bar is first applied to the oracle (oracle/ref_cpu.py) evaluated in
float32 against itself in float64, and tests/test_saturated_cpu.py asserts that the float32 oracle
stays inside half of it.  Where a case misses that, the inputs change, never the bar.

  1. head rows (head_case): 42 logit rows x 3 actions, one (V, R) pair per call, fed to the loss +
     head backward through one-hot fc activations, which lay every sample's dz bare in p_w / q_w;
  2. draw rows (draw_rows): spread 2 .. 2000, offsets 0 / +-3e4;
  3. LSTM (lstm_step_case, lstm_bptt_case): biases moved by +-20 / +-120, cell states to 1e3;
  4. engine parameters with the policy bias moved by +-100 (shifted_params)."""
import functools
import types

import numpy as np

from oracle import ref_cpu as R

EPS24 = 2.0 ** -24          # half an ulp of 1.0f: the relative error of one fp32 rounding
BETA = 0.01

# ------------------------------------------------------------------ 1. loss + head backward, per row
OFFSETS = (0.0, 1000.0, -1000.0)
# 17: 1 - pi is down to the last bits of 1.0f (0 for two actions); 90: exp is denormal; 104: the
# first gap where expf underflows to 0
GAPS = (1e-3, 10.0, 17.0, 30.0, 90.0, 104.0, 200.0, 1e4)
VR_PAIRS = ((0.0, 0.5), (100.0, 100.25), (-50.0, 50.0), (1e4, -1e4), (3.0, 3.0))
# literal_adv adds log pi(a) to dV, whose fp32 error at a peaked row is a rounding of sum exp >= 1,
# about 2^-24 whatever the advantage: the dV bar 4 x 2^-24 max(|adv|, |log pi(a)|) is checked on the
# pair whose advantage (100) puts the float32 oracle inside half of it
LITERAL_PAIR = (-50.0, 50.0)
N_ROWS = 42
N_SAMPLES = 3 * N_ROWS      # 126 <= 256, the narrower fc width: one one-hot column per sample


def logit_rows(A):
    """[42, A] float32: per offset the flat row, the flat row with logit 1 raised by each gap, and a
    two-way tie 50 ahead at actions 0 and A - 1; then four rows each of N(0, 1), N(0, 10), N(0, 100)."""
    rows = []
    for off in OFFSETS:
        rows.append(np.full(A, off))
        for gap in GAPS:
            r = np.full(A, off)
            r[1] += gap
            rows.append(r)
        r = np.full(A, off)
        r[0] += 50.0
        r[A - 1] += 50.0
        rows.append(r)
    rng = np.random.default_rng(1000 + A)
    for s in (1.0, 10.0, 100.0):
        rows.extend(rng.standard_normal((4, A)) * s)
    rows = np.asarray(rows).astype(np.float32)
    assert rows.shape == (N_ROWS, A)
    return rows


def head_case(A, V, Rt):
    """(z [126, A + 1] float32 with V in column A, actions [126] int32, target [126] float32): every
    row of logit_rows with its argmax, its argmin and action 2 (sample 3 r + k)."""
    rows = logit_rows(A)
    z = np.repeat(np.concatenate([rows, np.full((N_ROWS, 1), V, np.float32)], axis=1), 3, axis=0)
    actions = np.stack([rows.argmax(1), rows.argmin(1), np.full(N_ROWS, 2)], axis=1).reshape(-1).astype(np.int32)
    target = np.full(N_SAMPLES, Rt, np.float32)
    assert z.shape == (N_SAMPLES, A + 1) and float(np.float32(V)) == V and float(np.float32(Rt)) == Rt
    return z, actions, target


def loss_dz(z, actions, target, literal, dtype):
    """ref_cpu.a3c_loss_and_dz in `dtype`."""
    with np.errstate(over='ignore', under='ignore'):
        return R.a3c_loss_and_dz(z.astype(dtype), actions, target.astype(dtype), BETA, literal)


def row_scale(A, V, Rt):
    """What a row's dz is measured against: its advantage, or the entropy term's beta ln A."""
    return max(abs(Rt - V), BETA * np.log(A))


def row_ratios(dz, dz64, A, V, Rt):
    """Per sample: max over the A logit columns of |dz - dz64|, in units of 2^-24 x row_scale."""
    err = np.abs(np.asarray(dz, np.float64)[:, :A] - dz64[:, :A]).max(axis=1)
    return err / (EPS24 * row_scale(A, V, Rt))


@functools.lru_cache(maxsize=None)
def r32(A):
    """The float32 oracle's own worst row ratio over the five (V, R) pairs (4.3 at A = 6, 2.0 at
    A = 18 where this was written); the kernels' bar is four times it, the margin for the wave-tree
    summation order and the device's expf / logf."""
    worst = 0.0
    for V, Rt in VR_PAIRS:
        z, actions, target = head_case(A, V, Rt)
        _, dz64 = loss_dz(z, actions, target, False, np.float64)
        _, dz32 = loss_dz(z, actions, target, False, np.float32)
        assert np.isfinite(dz64).all() and np.isfinite(dz32).all()
        worst = max(worst, float(row_ratios(dz32, dz64, A, V, Rt).max()))
    return worst


def dv_bound(z, actions, target):
    """The literal_adv bar on dV per sample: 4 x 2^-24 x max(|adv|, |log pi(a)|)."""
    A = z.shape[1] - 1
    z64 = z.astype(np.float64)
    _, logpi, _ = R.softmax_stats(z64[:, :A])
    lpa = logpi[np.arange(len(actions)), actions]
    return 4 * EPS24 * np.maximum(np.abs(target.astype(np.float64) - z64[:, A]), np.abs(lpa))


def one_hot(B, width):
    """fc activations [B, width] with 1.0 at column b of row b: the head weight gradient's row b is
    then sample b's dz (the GEMM adds exact zeros), and only feature b passes the fc ReLU."""
    assert B <= width
    h = np.zeros((B, width), np.float32)
    h[np.arange(B), np.arange(B)] = 1.0
    return h


def q_case(A):
    """Q rows and targets to 1e4 for the q head's loss (z [126, A], actions, target): the rows and
    actions of head_case, scaled so that the widest row (offset 1000 + gap 1e4) peaks at 1e4, the
    targets cycling through magnitudes 0.5 .. 1e4 of both signs."""
    rows = logit_rows(A)
    z = np.repeat(rows * np.float32(1e4 / 11000.0), 3, axis=0).astype(np.float32)
    actions = np.stack([rows.argmax(1), rows.argmin(1), np.full(N_ROWS, 2)], axis=1).reshape(-1).astype(np.int32)
    target = np.resize(np.array([0.5, -1e4, 100.25, 1e4, -50.0, 3.0, 1000.0], np.float32), N_SAMPLES)
    assert np.abs(z).max() <= 1e4 * (1 + 1e-6) and np.abs(z).max() > 9e3
    return z, actions, target


def same_act_fwd(dqn_type, planes, acts, z, h3):
    """The oracle's forward record on given activations (acts: 'l1', 'l2' and, nature, 'l3' as
    [B, -1] arrays) with the head rows z [B, zw] and the fc output h3 put in their place."""
    B = planes.shape[0]
    f = {k: np.asarray(v, np.float64) for k, v in acts.items()}
    x0 = R.states_nhwc(planes).astype(np.float64) / 255.0
    if dqn_type == 'nature':
        layers = [x0, f['l1'].reshape(B, 20, 20, 32), f['l2'].reshape(B, 9, 9, 64), f['l3'].reshape(B, 7, 7, 64)]
        flat = f['l3'].reshape(B, -1)
    else:
        layers = [x0, f['l1'].reshape(B, 20, 20, 16), f['l2'].reshape(B, 9, 9, 32)]
        flat = f['l2'].reshape(B, -1)
    return dict(z=np.asarray(z, np.float64), h3=np.asarray(h3, np.float64), flat=flat, acts=layers)


def cast_fwd(fwd, dtype):
    return dict(z=fwd['z'].astype(dtype), h3=fwd['h3'].astype(dtype), flat=fwd['flat'].astype(dtype),
                acts=[a.astype(dtype) for a in fwd['acts']])


def oracle_loss_backward(p, fwd, algo, dqn_type, actions, target, literal):
    """Losses (the kernels' order) and gradients of the oracle on the record fwd, in fwd's dtype."""
    dt = fwd['z'].dtype.type
    with np.errstate(over='ignore', under='ignore'):
        if algo == 'a3c':
            losses, dz = R.a3c_loss_and_dz(fwd['z'], actions, target.astype(dt), BETA, literal)
            ref_loss = [losses['policy'], losses['value'], losses['entropy'], losses['total']]
        else:
            loss, dz = R.q_loss_and_dz(fwd['z'], actions, target.astype(dt))
            ref_loss = [loss, fwd['z'][np.arange(len(actions)), actions].mean()]
        return R.backward(p, fwd, dz, algo, dqn_type), ref_loss, dz


@functools.lru_cache(maxsize=None)
def cpu_trunk(dqn_type, A, algo='a3c', seed=0):
    """Parameters, frames and the oracle's own float64 forward of 126 random states (the CPU test's
    stand-in for the kernels' forward)."""
    from _net_parity import make_params
    p = make_params(types.SimpleNamespace(names_shapes=R.param_shapes(A, algo, dqn_type)), seed=seed + A, scale=4.0)
    planes = np.random.default_rng(seed + 7).integers(0, 256, (N_SAMPLES, 4, 84, 84), dtype=np.uint8)
    fwd = R.forward(p, R.states_nhwc(planes), algo, dqn_type)
    acts = {f'l{i}': a.reshape(N_SAMPLES, -1) for i, a in enumerate(fwd['acts']) if i > 0}
    return p, planes, acts


# ------------------------------------------------------------------ 2. action draw
DRAW_B, DRAW_SEED, DRAW_TAU = 4096, 123, 77
DRAW_WIDTHS = [(2, None), (7, None), (8, None), (9, None), (18, None), (31, None), (18, 32)]


def draw_rows(A, zs):
    """(rng, z [4096, zs] float32): z[b, :A] = N(0, 1) s_b + o_b with s_b in {2, 20, 200, 2000} by
    b % 4 and o_b in {0, +3e4, -3e4} by (b // 4) % 3; 1e30 in every other column."""
    rng = np.random.default_rng(40 + A)
    b = np.arange(DRAW_B)
    s = np.array([2.0, 20.0, 200.0, 2000.0])[b % 4]
    o = np.array([0.0, 3e4, -3e4])[(b // 4) % 3]
    z = np.full((DRAW_B, zs), 1e30, np.float32)
    z[:, :A] = (rng.standard_normal((DRAW_B, A)) * s[:, None] + o[:, None]).astype(np.float32)
    return rng, z


def draw_reference(z, A):
    """(a_ref, near, u, x): ref_cpu.sample_categorical on the fp64 softmax of z[:, :A] with the
    draw's Philox words, and the rows whose u lies within 1e-5 of a CDF boundary."""
    from oracle import philox as px
    x = px.philox4x32(DRAW_TAU, 0, np.arange(DRAW_B, dtype=np.uint32), px.P_ACTION, *px.seed_key(DRAW_SEED))
    pi, _, _ = R.softmax_stats(z[:, :A].astype(np.float64))
    u = px.u01(x[0])
    a_ref = R.sample_categorical(pi.astype(np.float32), u)
    near = np.min(np.abs(np.cumsum(pi, axis=1) - u[:, None].astype(np.float64)), axis=1) < 1e-5
    return a_ref, near, u, x


def top_gap(z, A):
    s = np.sort(z[:, :A].astype(np.float64), axis=1)
    return s[:, -1] - s[:, -2]


def unshifted_softmax32(logits):
    """What a kernel without the max-shift computes: fp32 exp(z) / sum exp(z), NaN read as 0."""
    with np.errstate(over='ignore', under='ignore', invalid='ignore', divide='ignore'):
        e = np.exp(np.asarray(logits, np.float32))
        return np.nan_to_num(e / e.sum(axis=1, keepdims=True), nan=0.0, posinf=0.0).astype(np.float32)


# ------------------------------------------------------------------ 3. LSTM cell and BPTT
U = 256
BIAS_LEVELS = np.array([0.0, 0.0, 20.0, -20.0, 120.0, -120.0, 0.0, 0.0], np.float32)
GATES = ('i', 'j', 'f', 'o')


def lstm_params(seed):
    """test_gpu_lstm._lstm_params with a level of BIAS_LEVELS added to every bias column: sigmoid
    reaches 1.0f at +20 and 0.0f at -120 (through exp = inf), tanh +-1.0f at +-20."""
    from test_gpu_lstm import _lstm_params
    w, b = _lstm_params(seed)
    rng = np.random.default_rng(seed + 5000)
    return w, (b + rng.choice(BIAS_LEVELS, b.shape[0])).astype(np.float32)


def lstm_step_case(B):
    """Inputs of one cell step (w, b, x, h, c, terms): c_prev = N(0, 1) x {0.5, 0.5, 30, 1e3} by b % 4."""
    rng = np.random.default_rng(B)
    w, b = lstm_params(B)
    x = np.maximum(rng.standard_normal((B, 256)), 0).astype(np.float32)
    h = (rng.standard_normal((B, U)) * 0.5).astype(np.float32)
    cs = np.array([0.5, 0.5, 30.0, 1e3])[np.arange(B) % 4]
    c = (rng.standard_normal((B, U)) * cs[:, None]).astype(np.float32)
    terms = (rng.random(B) < 0.3).astype(np.uint8)
    return w, b, x, h, c, terms


def lstm_step_oracle(case, dtype=np.float64):
    w, b, x, h, c, terms = case
    keep = (1 - terms.astype(dtype))[:, None]
    with np.errstate(over='ignore', under='ignore'):
        return R.lstm_cell(x.astype(dtype), (h * keep).astype(dtype), (c * keep).astype(dtype), w.astype(dtype),
                           b.astype(dtype))


def lstm_bptt_inputs(n, E):
    """The sequence a BPTT runs over: the oracle's own fp64 forward from c0 = N(0, 1) x {0.3, 30} by
    e % 2, rounded to float32.  (prm, x, seq32 {HP, CP, G, C}, terms, dH)"""
    rng = np.random.default_rng(100 + E)
    w, b = lstm_params(E)
    prm = {'lstm_w': w, 'lstm_b': b}
    x = np.maximum(rng.standard_normal((n, E, 256)) - 0.3, 0).astype(np.float32)
    terms = (rng.random((n, E)) < 0.2).astype(np.uint8)
    h0 = (rng.standard_normal((E, U)) * 0.3).astype(np.float32)
    cs = np.array([0.3, 30.0])[np.arange(E) % 2]
    c0 = (rng.standard_normal((E, U)) * cs[:, None]).astype(np.float32)
    with np.errstate(over='ignore', under='ignore'):
        seq = R.lstm_forward_seq(prm, x.astype(np.float64), h0.astype(np.float64), c0.astype(np.float64), terms)
    seq32 = {k: seq[k].astype(np.float32) for k in ('HP', 'CP', 'G', 'C')}
    dH = rng.standard_normal((n, E, U)).astype(np.float32)
    return prm, x, seq32, terms, dH


def lstm_bptt_oracle(inputs, dtype=np.float64):
    """(dX masked by x > 0, dW, dB) of ref_cpu.lstm_backward_seq on the float32 sequence, in dtype."""
    prm, x, seq32, terms, dH = inputs
    s = {k: v.astype(dtype) for k, v in seq32.items()}
    with np.errstate(over='ignore', under='ignore'):
        dX, dW, dB = R.lstm_backward_seq(prm, s, x.astype(dtype), dH.astype(dtype), terms)
    return dX * (x > 0), dW, dB


def saturated_shares(gates):
    """Per gate (i, j, f, o) of activated gates [..., 4 U]: the share that is exactly 0.0 or +-1.0
    in float32."""
    g = np.asarray(gates).astype(np.float32).reshape(-1, 4, U)
    sat = (g == 0.0) | (np.abs(g) == 1.0)
    return [float(sat[:, k].mean()) for k in range(4)]


def assert_gate_coverage(gates, tag):
    """At least 30 % of each gate's activations saturated, and at least 30 % not."""
    shares = saturated_shares(gates)
    for name, s in zip(GATES, shares):
        assert 0.3 <= s <= 0.7, (tag, name, s)
    return shares


# ------------------------------------------------------------------ 4. fused head kernels
SHIFTS = (100.0, -100.0)


def shifted_params(seed, scale, shift):
    """A build(params=...) callback: the usual init at 0.02 x scale with `shift` added to every
    element of p_b.  Softmax does not see a common offset, so every bar of the drivers holds; an
    unshifted expf gives inf / inf at +100 and, at -100, a five-bit denormal or 0 / 0."""
    def params(ns):
        from src.initializers import init_params
        p = init_params(ns, seed=seed, stddev=0.02 * scale)
        p['p_b'] = (p['p_b'] + np.float32(shift)).astype(np.float32)
        return p
    return params


def logit_recorder(A, seen):
    """A driver's start(eng, ref) hook that appends min |logit| of the oracle's own head rows to
    `seen`, once per replayed rollout."""
    def start(eng, ref):
        iterate = ref.iterate

        def recording(*args, **kw):
            out = iterate(*args, **kw)
            seen.append(float(np.abs(np.asarray(out['z'])[..., :A]).min()))
            return out
        ref.iterate = recording
    return start
