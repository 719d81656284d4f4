"""The cases of the op-tier stage test (test_op_stages_gpu.py) and, for every Linear case, what the library will launch for it —
without a GPU.  The coverage test_op_stage_cases_cpu.py asserts on the CPU is then the coverage the GPU test runs: the GPU test
holds the kernel a call reports (zg_debug_last_kernel, zg_debug_gemm_launches) to these predictions.

zg_linear_forward (api_ops.hip) takes one of two ways:

* batch >= 16, K % 64 == 0, K >= 128 (linear_mfma_ok, restated in mfma_ok): both fp32 operands are split into three bf16 planes
  and ONE matrix-core launch sums six plane products.  launch_gemm_planes picks the tile width and with it the kernel (restated in
  gemm_kernel): the four-wave gemm_s4_kernel for 192-wide tiles, the eight-wave gemm_p8_kernel<256> / <192> otherwise;
  ZGPT2_GEMM_KERNEL forces one; a ragged width (N % 4 != 0) is stored by the four-wave kernel only, whatever is forced; K = 16384
  is past the four-wave kernel's packed arguments and falls through to gemm_p8_kernel<192>.  The unforced choice is the four-wave
  kernel wherever the tiles of either width fit one round of 256 workgroups — the 256-wide choice needs more than 256 tiles of
  256 x 192 (M >= 16641 at N = 768), which is no seconds-sized case: the eight-wave kernels are reached by force.
* everything else: the GEMV kernels, planned per launch by gemv_plan.  gemv_launches() mirrors linear_device's row blocking
  (mb = 8, halved until (mb K + 8 mb + 64) 4 <= 160 KiB) and linear_device_wide's chunking beyond K = 8192 (the ragged chunk
  first, on the store epilogue; then whole chunks of 8192 through EPI_RESIDUAL onto y itself; W in row blocks of 2048; rows in
  blocks of 8 whatever K is) and asks zg_debug_gemv_plan for each launch.

What the plan says about two routes the issue of this test names:

* GR_VALU_GROUPS is NOT reachable through linear_device: its row blocks are sized by the same LDS formula the planner uses, so a
  block always fits.  It IS reached through the K chunks: linear_device_wide always takes blocks of 8 rows, and 5 .. 8 rows of a
  whole 8192-column chunk (mt = 8: 256.5 KiB) do not fit, so they run as two groups of 4 rows.  The M = 9 chunk cases cover it;
  test_op_stage_cases_cpu.py asserts both halves of this from the plan.
* Four-wave workgroups at M = 1 on GR_VALU are not reachable by a plain Linear: plan_valu gives a wave at least N / 2048 rows, so
  there are never more than 2048 waves, which is its threshold for one-wave workgroups; K in 2048 .. 8192 asks for two-wave
  workgroups, of which K % 32 == 0 goes to GR_KSPLIT instead.  The list has the one-wave form at a narrow and at the widest
  matrix (N = 50257 at K = 64) and the two-wave form (K = 2056); the CPU test asserts that these are all a sweep of the plan finds.

A yardstick Y is a maximum over the case's outputs: the cases keep at least eight outputs, and a hundred wherever the route allows.
"""
import ctypes as C
from dataclasses import dataclass

from test_gemv_plan_cpu import EPI_RESID, EPI_STORE, F32, FIELDS, PRO_NONE, RAGGED

from zig_gpt2_amd import _lib, synth

ROUTES = ["GR_VALU", "GR_VALU_GROUPS", "GR_GENERIC", "GR_KSPLIT"]  # what an fp32-weight plain Linear can plan (the first four of gemv.hip's)
GEMM_KERNELS = {"s4": "gemm_s4_kernel<3>, 6 pairs", "p8:192": "gemm_p8_kernel<192>, 6 pairs", "p8:256": "gemm_p8_kernel<256>, 6 pairs"}
MC_ROUTE = {"s4": "OP_S4", "p8:192": "OP_P8_192", "p8:256": "OP_P8_256"}  # names for stage_ref.bound_y
STAGING = 512 << 20   # zg_init's arena
K_CHUNK, W_ROWS = 8192, 2048
LDS_MAX = 160 * 1024


@dataclass(frozen=True)
class LinearCase:
    M: int
    K: int
    N: int
    bias: bool = True
    force: str = None     # ZGPT2_GEMM_KERNEL
    wgs: int = None       # ZGPT2_GEMM_WGS
    place: str = "host"   # operands: "host" numpy, "device" tensors, "registered" (host weight registered with the library)

    @property
    def id(self):
        return f"{self.M}x{self.K}x{self.N}" + ("" if self.bias else "-nobias") + (f"-{self.force}" if self.force else "") + \
            (f"-wgs{self.wgs}" if self.wgs else "") + ("" if self.place == "host" else f"-{self.place}")


# ---------------------------------------------------------------------------------------------- the matrix-core way
def mfma_ok(M, K, N, arena_left=STAGING // 2):
    """linear_mfma_ok.  arena_left: what the staged operands leave of the arena — the cases are a few MB, half the arena stands in."""
    if M < 16 or K < 128 or K % 64 != 0:
        return False
    if M * K * 3 >= 1 << 30 or N * K * 3 >= 1 << 30:
        return False
    if N % 4 != 0 and (K * 3 >= 65536 or K // 64 >= 256):
        return False
    return (M + N) * K * 3 * 2 + 1024 <= arena_left


def gemm_kernel(M, N, K, force=None):
    """launch_gemm_planes for the op tier's six pairs (lda = ldb = 3 K, ldc = N, fp32 output): "s4", "p8:192" or "p8:256"."""
    ragged = N % 4 != 0
    cost = lambda bn: ((((M + 255) // 256) * ((N + bn - 1) // bn) + 255) // 256) * bn
    bn = 192 if cost(192) * 8 <= cost(256) * 9 else 256
    if force in ("p8:192", "p8:256"):
        bn = int(force[3:])
    s4_ok = 3 * K < 65536 and N < 1 << 20 and K // 64 < 256  # gemm_s4_args_ok (six pairs are its most)
    assert s4_ok or not ragged
    if s4_ok and (force == "s4" or ragged or (not (force or "").startswith("p8") and bn == 192)):
        return "s4"
    return f"p8:{bn}"


def gemm_tiles(M, N, kernel):
    bn = 256 if kernel == "p8:256" else 192
    return ((M + 255) // 256) * ((N + bn - 1) // bn)


# ---------------------------------------------------------------------------------------------- the GEMV way
@dataclass(frozen=True)
class Launch:
    M: int
    N: int
    K: int
    epi: int
    bias: bool
    m0: int
    n0: int
    k0: int
    route: str
    plan: dict


def plan(M, N, K, epi, ragged_strides=False):
    out = (C.c_int * len(FIELDS))()
    _lib.check(_lib.load().zg_debug_gemv_plan(M, N, K, PRO_NONE, epi, F32, RAGGED if ragged_strides else 0, 0, 0, out, len(FIELDS)))
    return dict(zip(FIELDS, out))


def _launch(M, N, K, epi, bias, m0, n0, k0, out_f):
    p = plan(M, N, K, epi, ragged_strides=N != out_f)
    assert p["supported"], (M, N, K, epi)
    return Launch(M, N, K, epi, bias, m0, n0, k0, ROUTES[p["route"]], p)


def gemv_launches(M, K, N, bias=True):
    """The launches of linear_device_wide for an M x K input and an N x K weight, in order."""
    out = []
    if M == 0 or N == 0:
        return out
    if K <= K_CHUNK:  # linear_device
        mb = 8
        while mb > 1 and (mb * K + 8 * mb + 64) * 4 > LDS_MAX:
            mb >>= 1
        for m0 in range(0, M, mb):
            out.append(_launch(min(M - m0, mb), N, K, EPI_STORE, bias, m0, 0, 0, N))
        return out
    rows = min(W_ROWS, N)
    first = K % K_CHUNK or K_CHUNK
    for m0 in range(0, M, 8):
        k0 = 0
        while k0 < K:
            kc = first if k0 == 0 else K_CHUNK
            for n0 in range(0, N, rows):
                out.append(_launch(min(M - m0, 8), min(N - n0, rows), kc, EPI_STORE if k0 == 0 else EPI_RESID, bias and k0 == 0, m0, n0, k0, N))
            k0 += kc
    return out


def kernel_name(launch):
    """What zg_debug_last_kernel reports after this launch.  (GR_VALU_GROUPS: of its LAST group, which plan_valu lays out on its own.)"""
    p, r = launch.plan, launch.route
    if r == "GR_GENERIC":
        return "gemv_generic_kernel<float>"
    if r == "GR_KSPLIT":
        return f"gemv_ksplit_kernel<float, {p['lpr']}, {p['cpl']}, 2,"
    if r == "GR_VALU_GROUPS":
        g, last = p["row_group"], launch.M % p["row_group"] or p["row_group"]
        mt = 1 if last <= 1 else 2 if last <= 2 else 4 if last <= 4 else 8
        return f"gemv_kernel<float, {mt}, {p['lpr']}, {p['cpl']}, false>"
    return f"gemv_kernel<float, {p['mt']}, {p['lpr']}, {p['cpl']}, false>"


def route_of(case):
    """(route label, kernel-name prefix of the call's last launch, GEMM launches).  The label's first word is what stage_ref.bound_y reads."""
    if mfma_ok(case.M, case.K, case.N):
        k = gemm_kernel(case.M, case.N, case.K, case.force)
        return f"{MC_ROUTE[k]} six pairs, {gemm_tiles(case.M, case.N, k)} tiles" + (f" on {case.wgs} workgroups" if case.wgs else ""), GEMM_KERNELS[k], 1
    ls = gemv_launches(case.M, case.K, case.N, case.bias)
    names = []
    for l in ls:
        n = l.route + ("+resid" if l.epi == EPI_RESID else "")
        if n not in names:
            names.append(n)
    return " ".join(names) + f" ({len(ls)} launches)", kernel_name(ls[-1]), 0


def _cases():
    L = LinearCase
    c = [
        # ---- GEMV, fp32 weights, M < 16
        L(1, 768, 2304), L(1, 768, 2304, bias=False),    # GR_VALU, one-wave workgroups
        L(1, 64, 50257),                                 # the widest matrix: still one-wave workgroups (module docstring)
        L(1, 2056, 300),                                 # K >= 2048, K % 32 != 0: GR_VALU with two-wave workgroups
        L(1, 2048, 72), L(1, 8192, 264, bias=False),     # GR_KSPLIT at both ends of its range
        L(3, 768, 259), L(8, 1600, 64, bias=False), L(9, 384, 131),   # mt = 4, 8; row blocks of 8 + 1
        L(5, 8192, 40),                                  # mb drops to 4: blocks of 4 + 1, the single row on GR_KSPLIT
        L(4, 100, 37), L(2, 4108, 37, bias=False), L(4, 7, 37), L(8, 4108, 1), L(15, 100, 37),  # GR_GENERIC (K % 8 != 0), N % 4 != 0, N = 1
        L(3, 768, 259, place="device"), L(2, 4108, 37, place="device"), L(1, 2048, 72, place="registered"),
        # ---- K chunks
        L(1, 16384, 40),                                 # two whole chunks, the second GR_KSPLIT + EPI_RESIDUAL onto y
        L(3, 16384, 24, bias=False), L(9, 16384, 16),    # mt = 4 chunks; 8 + 1 rows: GR_VALU_GROUPS, then GR_KSPLIT
        L(1, 8192 + 579, 37), L(3, 8192 + 579, 37),      # a ragged chunk first, K % 8 != 0: GR_GENERIC feeds an accumulating chunk
        L(3, 8192 + 584, 37, bias=False),                # a ragged chunk that is a multiple of 8: GR_VALU feeds it
        L(9, 16389, 16, bias=False), L(5, 16389, 70),    # 5 ragged columns, then two whole chunks
        L(2, 8200, 2100),                                # crosses the 2048-row block of W
        L(3, 16384, 24, place="device"), L(1, 8192 + 579, 37, place="registered"),
    ]
    # ---- the six-product matrix-core Linear: every kernel by force and the unforced choice
    shapes = [(16, 128, 8), (127, 192, 192), (128, 768, 260), (129, 1600, 192), (257, 192, 260), (257, 768, 8), (16, 1600, 260), (128, 128, 192)]
    for force in (None, "s4", "p8:192", "p8:256"):
        c += [L(M, K, N, bias=(M + N) % 2 == 0, force=force) for M, K, N in shapes]
    # ragged widths: the four-wave kernel stores them, under any force
    c += [L(16, 128, 131), L(257, 192, 131, bias=False), L(129, 768, 193), L(127, 1600, 193, force="s4"), L(128, 192, 131, force="p8:256"),
          L(257, 768, 193, force="p8:192")]
    # one workgroup (three) walks several tiles with six pairs
    c += [L(257, 192, 260, force="s4", wgs=1), L(257, 768, 260, force="p8:256", wgs=3), L(257, 192, 260, force="p8:192", wgs=1), L(257, 768, 260, force="s4", wgs=3)]
    c += [L(16, 16384, 128)]                             # past s4's packed arguments: falls through to the eight-wave kernel
    c += [L(128, 768, 260, place="device"), L(129, 1600, 192, place="registered")]
    return c


LINEAR_CASES = _cases()
# the one shape test_op_stage_cases_cpu.py may exempt from the teeth assertion (it is measured and printed there all the same)
FALL_THROUGH = (16, 16384, 128)

LAYERNORM_CASES = [(1, 768), (3, 768), (7, 1600), (1, 5), (5, 64), (2, 4097)]   # rows x n; 4097: beyond the rows held in registers (2048)
GELU_SIZES = [1, 63, 64, 65, 3073, 100001]
SOFTMAX_SIZES = [1, 2, 63, 64, 65, 1024, 1025, 50257]
SDPA64_CASES = [(1, 12, 1), (1, 12, 64), (3, 2, 255), (1, 12, 256), (3, 2, 257), (1, 25, 513), (1, 12, 513), (3, 2, 64)]   # (b, h, T), head_dim 64
SDPA_ANY_CASES = [(4, 7, 19), (3, 32, 70), (2, 48, 300), (5, 80, 33), (1, 128, 513), (2, 300, 40), (1, 2048, 19), (2, 2048, 257)]  # (heads, head_dim, T)


def rows_for(n):
    """Independent rows (calls) of an elementwise case of n elements: enough for about 4096 outputs, 64 calls at the most."""
    return max(1, min(64, 4096 // n))


# ---------------------------------------------------------------------------------------------- operands (one draw per shape, shared by both tests)
def linear_operands(M, K, N):
    """x ~ N(0, 1), w ~ N(0, 0.05) UNROUNDED (the bits below bf16 are what the six products are for), bias ~ N(0, 0.05)."""
    return (synth.fill_normal(300 + M, M * K, 0, 1.0).reshape(M, K), synth.fill_normal(100 + N, N * K, 0, 0.05).reshape(N, K),
            synth.fill_normal(200 + N, N, 0, 0.05))


def layernorm_operands(rows, n):
    """Mean 0.3, standard deviation 2.0 (see test_op_stages_gpu.py on why no larger offset)."""
    return synth.fill_normal(7 + rows, rows * n, 0.3, 2.0).reshape(rows, n), synth.fill_normal(5, n, 1.0, 0.1), synth.fill_normal(6, n, 0.0, 0.1)


def attention_operands(b, h, T, d):
    return (synth.fill_normal(50 + T, b * h * d, 0, 1.0).reshape(b, h, d), synth.fill_normal(51 + T, b * h * T * d, 0, 1.0).reshape(b, h, T, d),
            synth.fill_normal(52 + T, b * h * T * d, 0, 1.0).reshape(b, h, T, d))
