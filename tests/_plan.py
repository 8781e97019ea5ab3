"""The backward's launch plans restated in plain Python.

Test infrastructure only.  The loss-and-backward path picks its launch shape from the batch size
B = n * E alone; the functions here restate those choices line for line from the C sources, and
tests/test_plan_cpu.py ties them to the library through the workspace sizes it reports (every
plan's `total` is what a3c_workspace_bytes / a3c_nature_workspace_bytes /
a3c_lstm_workspace_bytes size).  The GPU case tables (tests/test_gpu_batch_edges.py,
tests/test_gpu_lstm.py) assert from these functions that a batch reaches the fork it names, so
moving a plan constant fails a test instead of silently un-testing a fork.

Sources (async-rl-tensorflow_amd/csrc):
  gemm.hip   BM / BN / BK, a3c_gemm_plan_split, gemm_setup
  gemm.h     a3c_gemm_effective_split
  net.h      the NIPS trunk's geometry, PREP_BYTES, a3c_zs
  net_bwd.h  CB_SLAB
  net_bwd.hip  a3c_bwd_plan; k_conv_bwd's sample range; k_slab_group's slab range
  nature.h   the nature trunk's geometry, A3C_NAT_PREP_BYTES
  nature.hip   dw_split, nat_plan, fc_split, nat_fwd_slab_floats, a3c_nat_fwd_ws_floats
  lstm.hip   lstm_ws
The plans' A/B environment knobs (A3C_CB_NWG, A3C_NAT_DW_WGS*, A3C_NAT_FC_SPLIT) are taken at
their defaults."""
from collections import namedtuple

# gemm.hip:12-14
BM, BN, BK = 64, 64, 16

# net.h:14-36
HIST, IMG = 4, 84
C1_K, C1_N, C1_P = 8, 16, 400
C2_K, C2_N, C2_Q = 4, 32, 81
FLAT = C2_Q * C2_N                       # 2592
FC = 256
KC1 = C1_K * C1_K * HIST                 # 256
KC2 = C2_K * C2_K * C1_N                 # 256
LSTM_U = 256
LSTM_K = FC + LSTM_U
LSTM_G = 4 * LSTM_U
# net.h:180-186
W1S_ELEMS = C1_K * 3 * 64 * 8
PREP_W1S_BYTES = W1S_ELEMS * 2
PREP_W2F_OFF = PREP_W1S_BYTES + FLAT * FC * 4
W2F_ELEMS = 2 * 8 * 64 * 8
PREP_BYTES = PREP_W2F_OFF + W2F_ELEMS * 3 * 2
# net_bwd.h:8-12
CB_SLAB = KC1 * C1_N + KC2 * C2_N + C1_N + C2_N      # 12336
CB_NWG_MAX = 256                         # net_bwd.hip:999 (nwg_max)
CB_GROUPS_MAX = 16                       # net_bwd.hip:1020-1021
FC_WKS_MAXB = 2560                       # net_bwd.hip:977-981 fc_wks_on: the overlap engine's fc weight GEMM
#                                          splits K inside its workgroups (wg_split = 4) up to this B
LSTM_TILE = 16                         # lstm.hip LT: envs per k_lstm_fwd / k_lstm_bptt_step tile

# nature.h:10-25, 69-76
NT1_N, NT1_P, NT2_N, NT2_P, NT3_N, NT3_P = 32, 400, 64, 81, 64, 49
NT_K1, NT_K2, NT_K3 = 8 * 8 * HIST, 4 * 4 * NT1_N, 3 * 3 * NT2_N        # 256, 512, 576
NT_FLAT, NT_FC = NT3_P * NT3_N, 512
NT_A1, NT_A2 = NT1_P * NT1_N, NT2_P * NT2_N
NT_X2 = 4 * 4 * NT2_N
NAT_W2T_OFF = 3 * NT1_N * NT_K1 * 2
NAT_W3T_OFF = NAT_W2T_OFF + 3 * NT2_N * NT_K2 * 2
NAT_W2X_OFF = NAT_W3T_OFF + 3 * NT3_N * NT_K3 * 2
NAT_W3X_OFF = NAT_W2X_OFF + 3 * NT1_N * NT_X2 * 2
NAT_PREP_BYTES = NAT_W3X_OFF + 3 * NT2_N * NT_K3 * 2
NAT_GROUPS = 8                           # nature.hip:1383
NAT_DW_WGS = (768, 2048, 768)            # nature.hip:1408-1410
NAT_DW_MTILES = (2, 8, 9)                # nature.hip:1411-1413
NAT_FWD_SPLIT_MAX = 4                    # nature.hip:1446


def cdiv(a, b):
    return -(-a // b)


def zs(algo, A):
    """net.h:47-50 a3c_zs."""
    return ((A + 1 if algo == 'a3c' else A) + 3) & ~3


def gemm_plan_split(M, N, K, target_blocks):
    """gemm.hip:441-449 a3c_gemm_plan_split."""
    tiles = cdiv(M, BM) * cdiv(N, BN)
    ktiles = cdiv(K, BK)
    split = target_blocks // (tiles if tiles > 0 else 1)
    return min(max(split, 1), ktiles, 32)


def gemm_effective_split(K, nsplit):
    """gemm.h:55-61 a3c_gemm_effective_split."""
    if K < 1:
        return 1
    ktiles = cdiv(K, 16)
    per = cdiv(ktiles, max(nsplit, 1))
    return cdiv(ktiles, per)


def gemm_kchunk(K, nsplit):
    """gemm.hip:458-460 gemm_setup: the K rows of one split-K chunk (per * BK)."""
    return cdiv(cdiv(K, BK), max(nsplit, 1)) * BK


class Taker:
    """The plans' take(): 64-float aligned regions handed out in order."""

    def __init__(self):
        self.o = 0
        self.regions = []        # (name, offset, floats asked for)

    def __call__(self, name, floats):
        r = self.o
        self.regions.append((name, r, floats))
        self.o += (floats + 63) & ~63
        return r


BwdPlan = namedtuple('BwdPlan', 'B per_wg nwg groups per_group head_split fc_split_slab off regions total')


def bwd_plan(A, algo, B):
    """net_bwd.hip:983-1024 a3c_bwd_plan (+ per_group: a3c_backward_launch's `per` for k_slab_group,
    net_bwd.hip:1093)."""
    z = zs(algo, A)
    nwg = max(min(B, CB_NWG_MAX), 1)
    per_wg = cdiv(B, nwg)
    nwg = cdiv(B, per_wg)
    head_split = gemm_effective_split(B, gemm_plan_split(FC, z, B, 128))
    fc_split_slab = gemm_effective_split(B, gemm_plan_split(FLAT, FC, B, 512))
    take = Taker()
    off = dict(dz=take('dz', B * z), dh3=take('dh3', B * FC), dl2=take('dl2', B * FLAT),
               terms=take('terms', B * 4), hgrad=take('hgrad', FC * z), hcol=take('hcol', head_split * z),
               hslab=take('hslab', head_split * FC * z if head_split > 1 else 0),
               fccol=take('fccol', fc_split_slab * FC),
               fcslab=take('fcslab', fc_split_slab * FLAT * FC if fc_split_slab > 1 else 0),
               cslab=take('cslab', nwg * CB_SLAB))
    groups = min(nwg, CB_GROUPS_MAX)
    off['cgroup'] = take('cgroup', CB_GROUPS_MAX * CB_SLAB)
    return BwdPlan(B, per_wg, nwg, groups, cdiv(nwg, groups), head_split, fc_split_slab, off, take.regions, take.o)


def wg_samples(p, w):
    """k_conv_bwd (net_bwd.hip): workgroup w walks samples [w * per_wg, min(B, (w + 1) * per_wg))."""
    return min(p.B, (w + 1) * p.per_wg) - w * p.per_wg


def group_slabs(p, g):
    """k_slab_group (net_bwd.hip:832-840): group g folds slabs [g * per, min(nwg, (g + 1) * per))."""
    return max(min(p.nwg, (g + 1) * p.per_group) - g * p.per_group, 0)


def workspace_bytes(A, algo, B):
    """capi.hip:54-63 a3c_workspace_bytes."""
    return max(bwd_plan(A, algo, max(B, 1)).total, PREP_BYTES // 4) * 4 + 256


def dw_split(R, mtiles, target):
    """nature.hip:1389-1397 dw_split -> (ns, kc)."""
    want = max(target // mtiles, 1)
    per = cdiv(R, want)
    per = max(cdiv(per, 32) * 32, 32)
    return cdiv(R, per), per


NatPlan = namedtuple('NatPlan', 'B head_split ns kc off regions total')


def nat_plan(A, B):
    """nature.hip:1398-1436 nat_plan; ns / kc are the (conv1, conv2, conv3) triples."""
    z = zs('a3c', A)
    head_split = gemm_effective_split(B, gemm_plan_split(NT_FC, z, B, 128))
    sp = [dw_split(B * P, m, t) for P, m, t in zip((NT1_P, NT2_P, NT3_P), NAT_DW_MTILES, NAT_DW_WGS)]
    ns, kc = tuple(s[0] for s in sp), tuple(s[1] for s in sp)
    take = Taker()
    off = dict(dz=take('dz', B * z), dl4=take('dl4', B * NT_FC), dl3=take('dl3', B * NT_FLAT),
               dl2=take('dl2', B * NT_A2), dl1=take('dl1', B * NT_A1), terms=take('terms', B * 4),
               hgrad=take('hgrad', NT_FC * z), hcol=take('hcol', head_split * z),
               hslab=take('hslab', head_split * NT_FC * z if head_split > 1 else 0),
               fccol=take('fccol', NT_FC),
               s1=take('s1', ns[0] * NT_K1 * NT1_N), s2=take('s2', ns[1] * NT_K2 * NT2_N),
               s3=take('s3', ns[2] * NT_K3 * NT3_N),
               c1=take('c1', ns[0] * NT1_N), c2=take('c2', ns[1] * NT2_N), c3=take('c3', ns[2] * NT3_N),
               g1=take('g1', NAT_GROUPS * NT_K1 * NT1_N), g2=take('g2', NAT_GROUPS * NT_K2 * NT2_N),
               g3=take('g3', NAT_GROUPS * NT_K3 * NT3_N), wprep=take('wprep', NAT_PREP_BYTES // 4))
    return NatPlan(B, head_split, ns, kc, off, take.regions, take.o)


def nat_fc_split(B):
    """nature.hip:1438-1441 fc_split: the forward fc GEMM (M = B, N = 512, K = 3136)."""
    return gemm_effective_split(NT_FLAT, gemm_plan_split(B, NT_FC, NT_FLAT, 512))


def nat_fwd_ws_floats(B):
    """nature.hip:1465-1471 nat_fwd_slab_floats + the prepared weights."""
    sp = nat_fc_split(B)
    fc = sp * B * NT_FC if sp > 1 else 0
    cv = NAT_FWD_SPLIT_MAX * B * max(NT2_P * NT2_N, NT3_P * NT3_N)
    return cdiv(max(fc, cv), 64) * 64 + NAT_PREP_BYTES // 4


def nature_workspace_bytes(A, B):
    """nature.hip:1881-1888 a3c_nature_workspace_bytes."""
    return max(nat_fwd_ws_floats(B), nat_plan(A, B).total) * 4 + 256


LstmWs = namedtuple('LstmWs', 'n E split_dw off regions total')


def lstm_ws(n, E):
    """lstm.hip:274-286 lstm_ws."""
    nE = n * E
    split_dw = gemm_effective_split(nE, gemm_plan_split(FC, LSTM_G, nE, 256))
    take = Taker()
    off = dict(da=take('da', nE * LSTM_G), dcp=take('dcp', E * LSTM_U),
               slab=take('slab', split_dw * FC * LSTM_G if split_dw > 1 else 0),
               col=take('col', split_dw * LSTM_G))
    return LstmWs(n, E, split_dw, off, take.regions, take.o)


def lstm_workspace_bytes(n, E):
    """lstm.hip:352-356 a3c_lstm_workspace_bytes."""
    return lstm_ws(n, E).total * 4 + 256
