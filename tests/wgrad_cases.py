"""Cases, operand makers and the fp64 reference shared by tests/test_wgrad_cases_cpu.py and tests/test_gpu_wgrad_edges.py, and the
chunk-major converters that tests/test_gpu_round3.py uses too (no test in here).

The weight-gradient kernel (csrc/gemm.hip, wgrad_kernel) cuts the M rows of G = dY^T A into S splits of ``rows_per_split`` rows (a multiple
of 64) and walks each split in 64-row steps, unrolled by two over two register sets.  What a workgroup executes depends only on the number
of steps of its split and on the rows of the last one, so the cases are (M, S) pairs chosen by ``geometry``.  With small integer operands
every partial sum is an integer below 2^24: fp32 holds it exactly in any summation order, and the tests compare with ``torch.equal``."""
from functools import lru_cache

import torch
import torch.nn.functional as F

STEP = 64                # WG_MSTEP
PAD_ROWS = 6 * STEP      # NaN rows behind a row-major operand: further than any prefetch of the loop reaches (four steps ahead)
TOKENS = 197
NAN = float('nan')


def geometry(M, S):
    """The launch geometry of rovit_wgrad / rovit_wgrad_batch restated: one (m_begin, m_end, steps, tail_rows) per split.  ``tail_rows`` is
    the number of rows of the split's last step (64 = a full step); a split that starts at or past M is empty: (M, M, 0, 0)."""
    rows_per_split = ((M + S - 1) // S + STEP - 1) // STEP * STEP
    out = []
    for s in range(S):
        m_begin = s * rows_per_split
        m_end = min(M, m_begin + rows_per_split)
        if m_end <= m_begin:
            out.append((M, M, 0, 0))
            continue
        steps = (m_end - m_begin + STEP - 1) // STEP
        out.append((m_begin, m_end, steps, m_end - m_begin - (steps - 1) * STEP))
    return out


# (M, S): steps per split, rows of the last step of the last non-empty split
CASES = [
    (1, 1),        # 1; 1 row
    (63, 1),       # 1; 63
    (64, 1),       # 1; full
    (65, 1),       # 2; 1
    (129, 1),      # 3; 1
    (287, 1),      # 5; 31
    (353, 1),      # 6; 33
    (448, 1),      # 7; full
    (191, 2),      # 2 and 1; 63
    (192, 2),      # 2 and 1; full
    (193, 2),      # 2 and 2; 1
    (320, 2),      # 3 and 2; full
    (321, 2),      # 3 and 3; 1
    (449, 2),      # 4 and 4; 1
    (833, 2),      # 7 and 7; 1
    (895, 3),      # 5, 5 and 4; 63
    (130, 4),      # 1, 1, 1 (2 rows), empty
    (257, 4),      # 2, 2, 1 (1 row), empty
]

# The class-token launch: M = the batch, operand rows `stride` rows apart: (M, S, stride).  197 is the engine's stride (one class row per
# image); the larger batches use 3 to keep the operands small.
_CLS_SMALL = [(M, S, TOKENS) for M in (1, 2, 63, 64, 65) for S in sorted({1, min(4, (M + 63) // 64)})] + [(65, 4, TOKENS)]
_CLS_LARGE = [(M, S, 3) for M in (173, 256) for S in (1, min(4, (M + 63) // 64))]
CLS_CASES = _CLS_SMALL + _CLS_LARGE + [(M, S, 3) for M, S in CASES if M > 65]

# PatchEmbed rows: M = batch * 196, (batch, S)
PATCH_CASES = [(1, 1), (2, 1), (2, 2), (3, 4), (1, 8)]

# the linears of a transformer block as (N, K), in the order of the engine's merged launch
FC2, FC1, PROJ, QKV = (192, 768), (768, 192), (192, 192), (576, 192)
BLOCK_PROBLEMS = [FC2, FC1, PROJ, QKV]
SINGLE_SHAPES = [(192, 192), (576, 192), (192, 768), (96, 96)]
RANDN_CASE = (833, 2)
RANDN_PATCH_CASE = (4, 2)        # M = batch * 196 cannot be 833: 784 rows, 7 and 6 steps


# ------------------------------------------------------------------ operands ---------------------------------
def _gen(seed):
    return torch.Generator(device='cpu').manual_seed(seed)


@lru_cache(maxsize=None)
def int_operands(M, N, K, seed):
    """bf16 dY (M, N) with integers in [-2, 2] and A (M, K) with integers in [-3, 3] (different ranges: a transposed or swapped
    operand shows), CPU.  |sum| <= 6 M < 2^24 for every M the tests use."""
    g = _gen(seed)
    dY = torch.randint(-2, 3, (M, N), generator=g).to(torch.bfloat16)
    A = torch.randint(-3, 4, (M, K), generator=g).to(torch.bfloat16)
    return dY, A


@lru_cache(maxsize=None)
def randn_operands(M, N, K, seed):
    g = _gen(seed)
    return torch.randn(M, N, generator=g).to(torch.bfloat16), torch.randn(M, K, generator=g).to(torch.bfloat16)


def padded(t):
    """(M + PAD_ROWS, cols) allocation: the operand in rows [0, M), bf16 NaN behind it.  The kernel gets the view [:M]."""
    buf = torch.full((t.shape[0] + PAD_ROWS, t.shape[1]), NAN, dtype=t.dtype)
    buf[:t.shape[0]] = t
    return buf


def strided(t, r):
    """(M * r, cols) allocation: operand row m in row m * r (ld = cols * r), NaN in every row between."""
    buf = torch.full((t.shape[0] * r, t.shape[1]), NAN, dtype=t.dtype)
    buf[::r] = t
    return buf


def _rows(t, M):
    """chunk-major [cols / 32][M][32] (what the one-launch MLP kernels keep) -> row-major (M, cols)"""
    c = t.numel() // (M * 32)
    return t.view(c, M, 32).permute(1, 0, 2).reshape(M, c * 32).contiguous()


def _chunks(t):
    """row-major (M, cols) -> chunk-major [cols / 32][M][32], flat in the same (M, cols) shape"""
    M, cols = t.shape
    return t.view(M, cols // 32, 32).permute(1, 0, 2).contiguous().view(M, cols)


def _with_cls_rows(dy, batch):
    """(batch * 196, N) patch-row gradients -> (batch * 197, N) token rows whose class rows hold NaN"""
    N = dy.shape[1]
    dX = torch.full((batch, TOKENS, N), NAN, dtype=dy.dtype)
    dX[:, 1:] = dy.view(batch, TOKENS - 1, N)
    return dX.view(batch * TOKENS, N)


@lru_cache(maxsize=None)
def patch_operands(batch, N, seed, integer=True):
    """dX: bf16 (batch * 197, N) token-row gradients with NaN class rows; dy: its (batch * 196, N) patch rows; images: fp32 NCHW, values that
    bf16 holds exactly (integers in [-3, 3], or rounded normals); col: their bf16 (batch * 196, 768) im2col rows (conv k16 s16)."""
    g = _gen(seed)
    M = batch * (TOKENS - 1)
    if integer:
        dy = torch.randint(-2, 3, (M, N), generator=g).to(torch.bfloat16)
        images = torch.randint(-3, 4, (batch, 3, 224, 224), generator=g).float()
    else:
        dy = torch.randn(M, N, generator=g).to(torch.bfloat16)
        images = torch.randn(batch, 3, 224, 224, generator=g).to(torch.bfloat16).float()
    col = F.unfold(images, kernel_size=16, stride=16).transpose(1, 2).reshape(M, 768).to(torch.bfloat16)
    assert torch.equal(col.float().view(batch, 14, 14, 3, 16, 16)[0, 1, 2, 1, 3, 4], images[0, 1, 16 + 3, 32 + 4])
    return _with_cls_rows(dy, batch), dy, images, col


# ------------------------------------------------------------------ reference --------------------------------
def reference(dY, A, S):
    """fp64 on the CPU: per split s of geometry(M, S), G_s = dY[m_begin:m_end]^T A[m_begin:m_end] and colsum_s = dY[m_begin:m_end].sum(0)
    (zeros for an empty split); their sums over the splits.  Returns (slabs (S, N, K), colsums (S, N), G (N, K), colsum (N,))."""
    y, a = dY.double(), A.double()
    M = y.shape[0]
    slabs = torch.zeros(S, y.shape[1], a.shape[1], dtype=torch.float64)
    colsums = torch.zeros(S, y.shape[1], dtype=torch.float64)
    for s, (b, e, steps, _) in enumerate(geometry(M, S)):
        if steps:
            slabs[s] = y[b:e].t() @ a[b:e]
            colsums[s] = y[b:e].sum(0)
    return slabs, colsums, slabs.sum(0), colsums.sum(0)


_REF = {}


def int_reference(M, N, K, S, seed):
    """reference() of int_operands(M, N, K, seed), computed once per test session and shared (callers must not write to it)"""
    key = (M, N, K, S, seed)
    if key not in _REF:
        _REF[key] = reference(*int_operands(M, N, K, seed), S)
    return _REF[key]


def abs_bound(dY, A):
    """|dY|^T |A| (N, K) and |dY|.sum(0) (N,) in fp64: what the forward error bound of a sum in any order scales with"""
    y, a = dY.double().abs(), A.double().abs()
    return y.t() @ a, y.sum(0)
