"""CPU emulation of the bf16 term-split matrix passes (TEST INFRASTRUCTURE ONLY; imported by
tests/test_term_precision_cpu.py and tests/test_gpu_term_precision.py).

The hot path splits every fp32 operand into three round-to-nearest-even bf16 terms,
x = hi + mid + lo (net_fwd.hip split3_bits, nature.hip nat_split2 / nat_terms3, the dl1 split of
net_bwd.hip), and sums a fixed list of term products on the bf16 matrix cores:

  PRODUCTS6  hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi   (both operands fp32)
  PRODUCTS3  x.hi, x.mid, x.lo                              (one operand a u8 pixel: one exact term)

What is written here is that scheme in numpy (bf16_rn, split3, emulate), every layer of both trunks
as one matrix product C = A B with its epilogue (forward_case, backward_chain), and three
evaluations of a pass on given fp32 inputs:

  reference   A B in fp64
  honest      the same product as a plain fp32 FMA chain in sequential index order, followed by the
              roundings the kernels add after the sum (conv1's 1/255 on the accumulator, the bias
              add, the fp32 store) -- the worst case an fp32-class kernel is allowed
  mutant      the reference minus one second-order product A_i B_j (hi.lo, lo.hi, mid.mid; for a
              three-product pass the lo product) -- the scheme with that product missing

The bar of a pass is sqrt(e_honest * e_mut), e_mut the smallest mutant error, under the condition
e_mut >= 9 e_honest: at least 3x above the honest chain and 3x below the mildest mutant.  The
condition holds only where reductions are short (summation-order noise small, a dropped term as
large as ever), which is what sparse_params builds.  REAL_PASSES names the term-split passes.  The
passes that run on fp32 matrix instructions (the fc layers, the NIPS dW2 / dX2) or on plain FMAs
(the heads) have no product to lose and so no mutant; their bar is 3 x e_honest, the margin the
term-split bars keep above the honest chain at the least.

Errors are relative L2 of whole tensors (rel_err).  A forward entry whose fp64 pre-activation lies
within 1e-6 of zero may flip its ReLU under any rounding and is excluded; at most 0.1 % of a tensor
may be, and rel_err asserts that cap."""
import numpy as np

from oracle import ref_cpu as R

F32, F64 = np.float32, np.float64

PRODUCTS6 = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))
PRODUCTS3 = ((0, 0), (0, 1), (0, 2))
NNZ = 8                       # nonzero taps per conv output channel / rows per fc column
FLIP_EPS, FLIP_CAP = 1e-6, 1e-3

# the passes that are term products in a kernel (the others: fp32 MFMA / FMA, no mutants)
REAL_PASSES = {
    'nips': dict(fwd=('conv1', 'conv2'), bwd=('conv1_dW',)),
    'nature': dict(fwd=('conv1', 'conv2', 'conv3'),
                   bwd=('conv1_dW', 'conv2_dW', 'conv3_dW', 'conv2_dX', 'conv3_dX')),
}


# ---------------------------------------------------------------------------------------
# the number format
# ---------------------------------------------------------------------------------------
def bf16_bits(x):
    """Round-to-nearest-even bf16 of fp32 x, as the upper 16 bits (uint32).  NaN -> 0x7FC0, the
    value torch's conversion gives; an overflowing round carries into the exponent up to inf."""
    x = np.ascontiguousarray(x, F32)
    u = x.view(np.uint32)
    r = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)
    return np.where(np.isnan(x), np.uint32(0x7FC0), r).astype(np.uint32)


def bf16_rn(x):
    """x (fp32) rounded to the nearest bf16, returned as fp32."""
    return (bf16_bits(x) << np.uint32(16)).view(F32).reshape(np.shape(x))


def split3(x):
    """(hi, mid, lo) fp32 arrays: hi = bf16(x), mid = bf16(x - hi), lo = bf16((x - hi) - mid), the
    residuals formed in fp32 (exact: Sterbenz-like, each removes the leading 8 bits)."""
    x = np.asarray(x, F32)
    hi = bf16_rn(x)
    r1 = (x - hi).astype(F32)
    mid = bf16_rn(r1)
    r2 = (r1 - mid).astype(F32)
    return hi, mid, bf16_rn(r2)


def terms_of(x, n):
    """The n bf16 terms of fp32 x as fp64 arrays; n = 1 asserts x is exact in one term (u8 pixels)."""
    x = np.asarray(x, F32)
    if n == 1:
        assert np.array_equal(bf16_rn(x), x), 'a one-term operand must be exact in bf16'
        return [x.astype(F64)]
    return [t.astype(F64) for t in split3(x)]


def emulate(A_terms, B_terms, products):
    """The fp64 sum of the listed term products: sum over (i, j) of A_terms[i] @ B_terms[j]."""
    out = 0.0
    for i, j in products:
        out = out + A_terms[i] @ B_terms[j]
    return out


def products_of(na):
    return PRODUCTS3 if na == 1 else PRODUCTS6


def mutants_of(na):
    """name -> (i, j) of the second-order products: the ones whose absence costs ~2^-16 of a
    product, not 2^-8, and which the 1e-4 bars of the rest of the suite cannot see."""
    if na == 1:
        return {'lo': (0, 2)}
    return {'hi.lo': (0, 2), 'lo.hi': (2, 0), 'mid.mid': (1, 1)}


def chain_fp32(A, B):
    """A @ B as fp32 FMA chains in sequential k order: acc <- fl32(acc + a_k b_k) (the product of
    two fp32 is exact in fp64, so one fp64 add and one rounding to fp32 is the fused operation up
    to a double rounding of 2^-53)."""
    A = np.asarray(A, F32)
    B = np.asarray(B, F32)
    acc = np.zeros((A.shape[0], B.shape[1]), F32)
    A64, B64 = A.astype(F64), B.astype(F64)
    live = np.flatnonzero(np.any(A64 != 0, axis=0) & np.any(B64 != 0, axis=1))   # (a zero product adds exactly)
    for k in live:
        acc = (acc.astype(F64) + A64[:, k, None] * B64[None, k, :]).astype(F32)
    return acc


def rel_l2(a, b):
    a = np.asarray(a, F64)
    b = np.asarray(b, F64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---------------------------------------------------------------------------------------
# one pass = one matrix product + epilogue
# ---------------------------------------------------------------------------------------
class Case:
    """C = A B (A [M, K], B [K, N], fp32 values), na terms of A (1: u8 pixels), then
    out = act(C * scale + bias).  scale: conv1's 1/255 (the reference uses it in fp64, the honest chain
    as the fp32 constant the kernels multiply by); relu: the forward layers below the head."""

    def __init__(self, name, A, B, na=3, bias=None, scale=None, relu=False, real=False):
        self.name, self.na, self.relu, self.real = name, na, relu, real
        self.A = np.ascontiguousarray(A, F32)
        self.B = np.ascontiguousarray(B, F32)
        assert np.array_equal(self.A, np.asarray(A)) and np.array_equal(self.B, np.asarray(B)), 'operands are fp32'
        self.bias = None if bias is None else np.asarray(bias, F32)
        self.scale = scale

    def _post64(self, C):
        if self.scale is not None:
            C = C * F64(self.scale)
        if self.bias is not None:
            C = C + self.bias.astype(F64)
        return C

    def evaluate(self):
        """dict: pre (fp64 pre-activation), ref, honest, full (term-split pass: the documented
        product list summed exactly; otherwise the fp64 sum; stored as fp32), muts {name: output}
        (term-split passes only)."""
        A64, B64 = self.A.astype(F64), self.B.astype(F64)
        act = (lambda v: np.maximum(v, 0)) if self.relu else (lambda v: v)
        C = A64 @ B64
        pre = self._post64(C)
        h = chain_fp32(self.A, self.B)
        if self.scale is not None:
            h = (h * F32(self.scale)).astype(F32)
        if self.bias is not None:
            h = (h + self.bias).astype(F32)
        muts, full = {}, pre.astype(F32)
        if self.real:
            At, Bt = terms_of(self.A, self.na), terms_of(self.B, 3)
            full = self._post64(emulate(At, Bt, products_of(self.na))).astype(F32)
            muts = {m: act(self._post64(C - At[i] @ Bt[j])) for m, (i, j) in mutants_of(self.na).items()}
        return dict(pre=pre, ref=act(pre), honest=act(h), full=act(full), muts=muts)


def rel_err(out, ev, relu=True):
    """Relative L2 of `out` against ev['ref'] over the entries whose fp64 pre-activation is not
    within FLIP_EPS of zero (relu layers only); asserts that at most FLIP_CAP of the tensor is
    excluded.  Returns (error, excluded fraction)."""
    ref = ev['ref']
    out = np.asarray(out, F64).reshape(ref.shape)
    if not relu:
        return rel_l2(out, ref), 0.0
    keep = np.abs(ev['pre']) >= FLIP_EPS
    frac = 1.0 - float(keep.mean())
    assert frac <= FLIP_CAP, ('near-zero pre-activations excluded', frac)
    return rel_l2(out[keep], ref[keep]), frac


HONEST_MARGIN = 3.0     # the bar of a pass without term products: 3 x its honest fp32 chain


def bars_of(case, ev=None):
    """dict e_honest, e_full, e_mut (the smallest; None without mutants), e_muts {name: error}, bar.
    Term-split pass: bar = sqrt(e_honest e_mut).  A pass on fp32 instructions has no product to
    lose: its bar is HONEST_MARGIN x e_honest, the margin the term-split bars keep above the honest
    chain at the least (an fp32 sum in any order is in the error class of the sequential one)."""
    ev = case.evaluate() if ev is None else ev
    e_h = rel_err(ev['honest'], ev, case.relu)[0]
    e_f = rel_err(ev['full'], ev, case.relu)[0]
    e_ms = {m: rel_err(v, ev, case.relu)[0] for m, v in ev['muts'].items()}
    e_m = min(e_ms.values()) if e_ms else None
    bar = float(np.sqrt(e_h * e_m)) if case.real else HONEST_MARGIN * e_h
    return dict(e_honest=e_h, e_full=e_f, e_mut=e_m, e_muts=e_ms, bar=bar, real=case.real, ev=ev)


def assert_design(name, b):
    """The condition that makes sqrt(e_honest e_mut) a bar: 3x above honest, 3x below every mutant;
    and what the emulation must show: the full product list passes it, every mutant fails it."""
    assert b['e_honest'] > 0, name
    assert b['e_full'] <= b['bar'], (name, 'the full scheme misses its own bar', b['e_full'], b['bar'])
    if not b['real']:
        return
    assert b['e_mut'] >= 9.0 * b['e_honest'], (name, 'e_mut < 9 e_honest', b['e_honest'], b['e_mut'])
    assert len(b['e_muts']) in (1, 3)
    for m, e in b['e_muts'].items():
        assert e > b['bar'], (name, m, e, b['bar'])


def fmt(name, b, gpu=None):
    s = f"{name:<16} e_honest {b['e_honest']:.2e}  e_full {b['e_full']:.2e}  "
    if b['real']:
        s += f"e_mut {b['e_mut']:.2e} (x{b['e_mut'] / b['e_honest']:.0f})  bar {b['bar']:.2e}"
    else:
        s += f"(fp32 pass: no mutants)    bar {b['bar']:.2e}"
    return s if gpu is None else s + f'  gpu {gpu:.2e}'


# ---------------------------------------------------------------------------------------
# the two trunks, layer by layer
# ---------------------------------------------------------------------------------------
def fc_name(algo):
    return 'l4' if algo == 'a3c' else 'l3'


def head_wb(P, algo):
    """The head as one matrix: a3c [fc, A + 1] (policy columns, then the value), q [fc, A]."""
    if algo == 'a3c':
        return np.concatenate([P['p_w'], P['q_w']], axis=1), np.concatenate([P['p_b'], P['q_b']])
    return P['q_w'], P['q_b']


def layer_names(dqn_type):
    convs, _, _ = R.trunk_spec(dqn_type)
    return [f'conv{i + 1}' for i in range(len(convs))] + ['fc', 'head']


def forward_case(P, layer, x_in, algo, dqn_type):
    """The Case of one forward layer on the given input: conv1 takes u8 NHWC states [B,84,84,4],
    conv i > 1 the fp32 NHWC output of conv i-1, fc the flattened last conv output (or its NHWC
    form), head the fc output."""
    convs, flat, fc = R.trunk_spec(dqn_type)
    real = layer in REAL_PASSES[dqn_type]['fwd']
    if layer.startswith('conv'):
        i = int(layer[4:]) - 1
        c = convs[i]
        x = np.asarray(x_in)
        assert x.dtype == (np.uint8 if i == 0 else F32), (layer, x.dtype)
        x = np.ascontiguousarray(x.astype(F32).reshape(-1, c['ih'], c['iw'], c['cin']))
        A = R._patches(x, c['k'], c['s']).reshape(x.shape[0] * c['oh'] * c['ow'], -1)
        W = P[f'l{i + 1}_w'].reshape(-1, c['cout'])
        return Case(layer, A, W, na=1 if i == 0 else 3, bias=P[f'l{i + 1}_b'], scale=1.0 / 255.0 if i == 0 else None,
                    relu=True, real=real)
    if layer == 'fc':
        fcn = fc_name(algo)
        return Case(layer, np.asarray(x_in, F32).reshape(-1, flat), P[fcn + '_w'], bias=P[fcn + '_b'], relu=True)
    assert layer == 'head'
    W, b = head_wb(P, algo)
    return Case(layer, np.asarray(x_in, F32).reshape(-1, fc), W, bias=b)


def forward_emulated(P, states_u8, algo, dqn_type):
    """The forward evaluated layer by layer, each on the fp32-stored honest output of the layer
    below (what a kernel would be handed).  Returns (inputs {layer: x_in}, outs {layer: fp32 out})."""
    x = np.ascontiguousarray(states_u8, np.uint8)
    convs, _, _ = R.trunk_spec(dqn_type)
    ins, outs = {}, {}
    for layer in layer_names(dqn_type):
        case = forward_case(P, layer, x, algo, dqn_type)
        ins[layer] = x
        y = case.evaluate()['honest']
        if layer.startswith('conv'):
            c = convs[int(layer[4:]) - 1]
            y = y.reshape(-1, c['oh'], c['ow'], c['cout'])
        outs[layer] = x = np.ascontiguousarray(y, F32)
    return ins, outs


def fwd_record(P, states_u8, outs, algo, dqn_type):
    """ref_cpu.forward's record built from given layer outputs {conv1.., fc, head} (the GPU's, or
    forward_emulated's), so that ref_cpu.backward runs on exactly those activations and masks."""
    convs, flat, _ = R.trunk_spec(dqn_type)
    B = states_u8.shape[0]
    acts = [np.asarray(states_u8, F64) / 255.0]
    for i, c in enumerate(convs):
        acts.append(np.asarray(outs[f'conv{i + 1}'], F64).reshape(B, c['oh'], c['ow'], c['cout']))
    return dict(z=np.asarray(outs['head'], F64), h3=np.asarray(outs['fc'], F64).reshape(B, -1),
                flat=acts[-1].reshape(B, flat), acts=acts)


# ---------------------------------------------------------------------------------------
# the backward as a chain of matrix passes
# ---------------------------------------------------------------------------------------
def bwd_pass_names(dqn_type):
    """Top-down order of the trunk backward's matrix passes."""
    n = len(R.trunk_spec(dqn_type)[0])
    out = ['head_dX', 'fc_dW', 'fc_dX']
    for i in range(n, 0, -1):
        out.append(f'conv{i}_dW')
        if i > 1:
            out.append(f'conv{i}_dX')
    return out


def grad_feeds(algo, dqn_type):
    """trunk gradient tensor -> the passes whose products reach it: its own dW pass (weights) and
    every dX pass above it.  The backward's map from passes to tensors:
      head_dX -> everything;  fc_dW -> fc weights;  fc_dX -> every conv tensor;
      conv i dW -> l{i}_w;  conv i dX -> l{j}_w, l{j}_b for j < i."""
    n = len(R.trunk_spec(dqn_type)[0])
    fcn = fc_name(algo)
    feeds = {fcn + '_w': ['head_dX', 'fc_dW'], fcn + '_b': ['head_dX']}
    above = ['head_dX', 'fc_dX']
    for i in range(n, 0, -1):
        feeds[f'l{i}_w'] = above + [f'conv{i}_dW']
        feeds[f'l{i}_b'] = list(above)
        above = above + [f'conv{i}_dX']
    return feeds


def backward_chain(P, fwd, dz, algo, dqn_type, mm, rnd=lambda v: v):
    """ref_cpu.backward's trunk gradients with every matrix product routed through
    mm(name, A, B, scale) -> C (scale: conv1_dW's 1/255, applied to the sum as the kernels'
    finalize does) and every tensor a kernel would store passed through rnd.  With an fp64 mm it
    equals ref_cpu.backward (asserted in tests/test_term_precision_cpu.py)."""
    convs, flat, fc = R.trunk_spec(dqn_type)
    fcn = fc_name(algo)
    Wh, _ = head_wb(P, algo)
    dz = np.asarray(dz, F64)
    h3 = fwd['h3']
    g = {}
    dh3 = rnd(mm('head_dX', dz, Wh.T.astype(F64), None) * (h3 > 0))
    g[fcn + '_w'] = rnd(mm('fc_dW', fwd['flat'].T, dh3, None))
    g[fcn + '_b'] = rnd(dh3.sum(0))
    acts = fwd['acts']
    dx = mm('fc_dX', dh3, P[fcn + '_w'].T.astype(F64), None).reshape(acts[-1].shape)
    dx = rnd(dx * (acts[-1] > 0))
    for i in range(len(convs) - 1, -1, -1):
        c = convs[i]
        xin = acts[i]
        B = xin.shape[0]
        dy = dx.reshape(-1, c['cout'])
        if i == 0:      # patches of the unscaled u8 pixels, 1/255 on the sum
            pix = np.ascontiguousarray(np.rint(xin * 255.0))
            p = R._patches(pix, c['k'], c['s']).reshape(B * c['oh'] * c['ow'], -1)
            g['l1_w'] = rnd(mm('conv1_dW', p.T, dy, 1.0 / 255.0)).reshape(c['k'], c['k'], c['cin'], c['cout'])
            g['l1_b'] = rnd(dy.sum(0))
            break
        p = R._patches(xin, c['k'], c['s']).reshape(B * c['oh'] * c['ow'], -1)
        g[f'l{i + 1}_w'] = rnd(mm(f'conv{i + 1}_dW', p.T, dy, None)).reshape(c['k'], c['k'], c['cin'], c['cout'])
        g[f'l{i + 1}_b'] = rnd(dy.sum(0))
        w = P[f'l{i + 1}_w'].astype(F64).reshape(-1, c['cout'])
        dp = mm(f'conv{i + 1}_dX', dy, w.T, None).reshape(B, c['oh'], c['ow'], c['k'], c['k'], c['cin'])
        dxin = np.zeros_like(xin)
        s = c['s']
        for kh in range(c['k']):
            for kw in range(c['k']):
                dxin[:, kh:kh + s * c['oh']:s, kw:kw + s * c['ow']:s, :] += dp[:, :, :, kh, kw, :]
        dx = rnd(dxin * (xin > 0))
    return g


def mm_fp64(name, A, B, scale):
    C = np.asarray(A, F64) @ np.asarray(B, F64)
    return C if scale is None else C * scale


def f32r(v):
    return np.asarray(v, F32).astype(F64)


def mm_honest(name, A, B, scale):
    C = chain_fp32(np.asarray(A, F32), np.asarray(B, F32))
    if scale is not None:
        C = (C * F32(scale)).astype(F32)
    return C.astype(F64)


def na_of(name):
    return 1 if name == 'conv1_dW' else 3


def mm_full(dqn_type):
    """Term-split passes: the documented product list of the fp32 operands summed exactly; the
    others: the fp64 product; either stored as fp32."""
    def mm(name, A, B, scale):
        A, B = np.asarray(A, F32), np.asarray(B, F32)
        if name in REAL_PASSES[dqn_type]['bwd']:
            C = emulate(terms_of(A, na_of(name)), terms_of(B, 3), products_of(na_of(name)))
        else:
            C = A.astype(F64) @ B.astype(F64)
        return f32r(C if scale is None else C * scale)
    return mm


def mm_drop(pass_name, ij):
    """fp64 products, except that pass `pass_name` is A B - A_i B_j (terms of the fp32 operands)."""
    def mm(name, A, B, scale):
        C = np.asarray(A, F64) @ np.asarray(B, F64)
        if name == pass_name:
            At, Bt = terms_of(np.asarray(A, F32), na_of(name)), terms_of(np.asarray(B, F32), 3)
            C = C - At[ij[0]] @ Bt[ij[1]]
        return C if scale is None else C * scale
    return mm


def backward_cases(P, fwd, dz, algo, dqn_type):
    """{pass: Case} of every backward pass in isolation, on the fp32-stored operands the fp64 chain
    hands it."""
    cases = {}

    def mm(name, A, B, scale):
        cases[name] = Case(name, np.asarray(A, F32), np.asarray(B, F32), na=na_of(name),
                           scale=scale, real=name in REAL_PASSES[dqn_type]['bwd'])
        return mm_fp64(name, A, B, scale)
    backward_chain(P, fwd, dz, algo, dqn_type, mm, rnd=f32r)
    return cases


def backward_bars(P, fwd, dz, algo, dqn_type):
    """(pass_bars {pass: bars_of}, tensor_bar, tensor_honest {tensor: the error of the whole backward
    run as honest fp32 chains}).  A tensor fed by term-split passes takes the smallest bar among
    them; one fed by fp32 passes only takes HONEST_MARGIN x its error in the honest chain."""
    pb = {name: bars_of(c) for name, c in backward_cases(P, fwd, dz, algo, dqn_type).items()}
    g_ref = backward_chain(P, fwd, dz, algo, dqn_type, mm_fp64)
    th = grads_err(backward_chain(P, fwd, dz, algo, dqn_type, mm_honest, rnd=f32r), g_ref)
    tb = {}
    for t, feeds in grad_feeds(algo, dqn_type).items():
        real = [pb[p]['bar'] for p in feeds if pb[p]['real']]
        tb[t] = min(real) if real else HONEST_MARGIN * th[t]
    return pb, tb, th


def grads_err(g, g_ref):
    return {k: rel_l2(np.asarray(g[k]).reshape(-1), np.asarray(g_ref[k]).reshape(-1)) for k in g_ref if k in g}


def backward_mutants(P, fwd, dz, algo, dqn_type, g_ref, passes=None):
    """{(pass, mutant): {tensor: error}}: the pass's product dropped in fp64 and propagated through
    the layers below it, against the unmutated fp64 gradients g_ref."""
    out = {}
    for name in (REAL_PASSES[dqn_type]['bwd'] if passes is None else passes):
        for m, ij in mutants_of(na_of(name)).items():
            out[(name, m)] = grads_err(backward_chain(P, fwd, dz, algo, dqn_type, mm_drop(name, ij)), g_ref)
    return out


# ---------------------------------------------------------------------------------------
# short-chain inputs
# ---------------------------------------------------------------------------------------
def sparse_params(names_shapes, algo, dqn_type, seed):
    """Parameters whose reductions are short: every conv output channel has NNZ nonzero taps at
    random (kh, kw, cin), every fc column NNZ nonzero rows, all within two spatial positions of the
    flattened last conv output (so dl of that layer is nonzero at two positions and the dW
    reductions over positions stay short at B = 1); the head is dense.  Each layer is scaled on a
    probe batch so that its pre-activation rms is 1 (activation rms then lies well inside
    [0.05, 5]); biases are N(0.1, 0.1)."""
    rng = np.random.default_rng(seed)
    convs, flat, fc = R.trunk_spec(dqn_type)
    shapes = dict(names_shapes)
    P = {}
    x = rng.integers(0, 256, (2, 84, 84, 4), dtype=np.uint8).astype(F64) / 255.0
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))   # noqa: E731

    def bias(n):
        return (0.1 + 0.1 * rng.standard_normal(n)).astype(F32)

    for i, c in enumerate(convs):
        K = c['k'] * c['k'] * c['cin']
        w = np.zeros((K, c['cout']))
        for o in range(c['cout']):
            w[rng.choice(K, NNZ, replace=False), o] = rng.standard_normal(NNZ)
        p = R._patches(np.ascontiguousarray(x), c['k'], c['s']).reshape(-1, K)
        w = (w / rms(p @ w)).astype(F32)
        b = bias(c['cout'])
        P[f'l{i + 1}_w'], P[f'l{i + 1}_b'] = w.reshape(shapes[f'l{i + 1}_w']), b
        x = np.maximum(p @ w.astype(F64) + b, 0).reshape(2, c['oh'], c['ow'], c['cout'])
    last = convs[-1]
    h = x.reshape(2, flat)
    live = (h > 0).all(axis=0).reshape(last['oh'] * last['ow'], last['cout'])      # on in both probe samples
    pos = np.argsort(-live.sum(1), kind='stable')[:2]                              # the two liveliest positions
    rows = np.concatenate([p * last['cout'] + np.flatnonzero(live[p]) for p in pos])
    assert rows.size >= 2 * NNZ, rows.size
    w = np.zeros((flat, fc))
    for o in range(fc):
        w[rng.choice(rows, NNZ, replace=False), o] = rng.standard_normal(NNZ)
    w = (w / rms(h @ w)).astype(F32)
    fcn = fc_name(algo)
    P[fcn + '_w'], P[fcn + '_b'] = w, bias(fc)
    h3 = np.maximum(h @ w.astype(F64) + P[fcn + '_b'], 0)
    heads = [k for k, _ in names_shapes if k in ('p_w', 'q_w')]
    for k in heads:
        wk = rng.standard_normal(shapes[k])
        P[k] = (wk / rms(h3 @ wk)).astype(F32)
        P[k[0] + '_b'] = (0.1 * rng.standard_normal(shapes[k[0] + '_b'])).astype(F32)
    assert set(P) == set(shapes), (sorted(P), sorted(shapes))
    return P


def dense_states(B, seed):
    """[B,4,84,84] u8 planes, dense random."""
    return np.random.default_rng(seed).integers(0, 256, (B, 4, 84, 84), dtype=np.uint8)


def assert_alive(name, act):
    """An all-zero layer would pass anything: rms in [0.05, 5], at least 25 % nonzero."""
    a = np.asarray(act, F64)
    r = float(np.sqrt(np.mean(a * a)))
    nz = float((a != 0).mean())
    assert 0.05 <= r <= 5.0, (name, 'activation rms', r)
    assert nz >= 0.25, (name, 'nonzero fraction', nz)
    return r, nz


# ---------------------------------------------------------------------------------------
# the checks shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------
def forward_check(P, states_u8, outs, algo, dqn_type, layers=None):
    """Layer-isolated: every layer of `outs` {conv1.., fc, head} (fp32) against that layer in fp64
    on outs' own input activations.  Returns {layer: (bars_of, error of outs[layer], case)}."""
    names = layer_names(dqn_type)
    res = {}
    for li, layer in enumerate(names):
        if layers is not None and layer not in layers:
            continue
        x_in = states_u8 if li == 0 else np.asarray(outs[names[li - 1]], F32)
        case = forward_case(P, layer, x_in, algo, dqn_type)
        b = bars_of(case)
        res[layer] = (b, rel_err(outs[layer], b['ev'], case.relu)[0], case)
    return res


def backward_check(P, states_u8, outs, dz, algo, dqn_type):
    """On the activations `outs` (their ReLU masks) and the head gradient dz: the fp64 oracle
    gradients (ref_cpu.backward), the per-pass bars, the per-tensor bars and the propagated mutants
    of the term-split passes.  Returns dict fwd, dz, g_ref, pass_bars, tensor_bar, tensor_honest, mutants."""
    fwd = fwd_record(P, states_u8, outs, algo, dqn_type)
    dz = np.asarray(np.asarray(dz, F32), F64)
    g_ref = R.backward(P, fwd, dz, algo, dqn_type)
    pb, tb, th = backward_bars(P, fwd, dz, algo, dqn_type)
    muts = backward_mutants(P, fwd, dz, algo, dqn_type, g_ref)
    return dict(fwd=fwd, dz=dz, g_ref=g_ref, pass_bars=pb, tensor_bar=tb, tensor_honest=th, mutants=muts)


def assert_mutants_caught(chk, tag):
    """Every mutant of every term-split pass moves at least one gradient tensor beyond its bar."""
    for (name, m), errs in chk['mutants'].items():
        hit = [t for t, e in errs.items() if t in chk['tensor_bar'] and e > chk['tensor_bar'][t]]
        assert hit, (tag, name, m, 'moves no tensor beyond its bar', errs, chk['tensor_bar'])
