"""Cases shared by the CPU and GPU tests of the ragged-batch forward (tests/test_ragged_cpu.py, tests/test_gpu_ragged.py)."""
import numpy as np

# sequence lengths at the edges of attn_fwd_ragged_kernel: the 16-query tile (15, 16, 17), the 32 rows a wave owns and the 32-key P V
# block (31, 32, 33, 64, 65), a second key tile inside a block (48, 49), the last key tile (196, 197), the class token alone (1, 2)
L = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 196, 197)
# L in a fixed shuffled order (a permutation written out, so the cases do not depend on a generator)
L_SHUFFLED = (33, 1, 197, 16, 64, 2, 49, 15, 196, 65, 17, 32, 48, 31)
assert sorted(L_SHUFFLED) == list(L)


def cycle_lengths(n: int):
    """n lengths cycling through the shuffled L."""
    return [L_SHUFFLED[i % len(L_SHUFFLED)] for i in range(n)]


def offsets_of(lengths) -> np.ndarray:
    """(n + 1,) int32 row offsets of sequences packed in the given order."""
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int32)


def layout_reference(lengths, max_rows: int):
    """ragged_layout by the plainest loop: longest first (stable), a call closed when the next sequence would pass max_rows."""
    order = sorted(range(len(lengths)), key=lambda i: -lengths[i])
    calls, cur, rows = [], [], 0
    for i in order:
        if cur and rows + lengths[i] > max_rows:
            calls.append(cur)
            cur, rows = [], 0
        cur.append(i)
        rows += lengths[i]
    calls.append(cur)
    return calls
