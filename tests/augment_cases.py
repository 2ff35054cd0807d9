"""The case table of the translate kernel's path tests (tests/test_augment_paths_cpu.py, tests/test_gpu_augment_paths.py): one call of
tg_random_translate per case, built at the edges of the launcher's path decision (csrc/tg_augment.h: translate_plan) and of the kernel's span
arithmetic (csrc/tg_augment.hip: k_random_translate).

A case is (dtype, channels_first, C, H, W, B, input-offset bytes, output-offset bytes, params recipe) plus the path class it is in the table
for.  The offsets are added to 16-byte aligned addresses inside larger buffers.  The params recipe is `explicit` (explicit_rows(H, W) followed
by draws, so that every case carries every shift class) with the explicit rows first or - for the cases of more than one launch - last, where
the second launch then finds them.  Everything is deterministic: inputs and draws are functions of the case alone.
"""
import collections

import numpy as np

from augment_ref import draw_params

CHUNK = 4096          # kAugChunk: output elements per workgroup
MAX_ROW = 8192        # kTrMaxRow: R + S of the staged path
MAX_BLOCKS = 1 << 23  # workgroups per launch

# The path classes: every one must keep a case for each of the four kernel instantiations (uint8 / float32 x channels first / last).
CLASSES = ("staged_single", "staged_whole", "staged_ragged", "elem_plane", "elem_in", "elem_out", "elem_row", "multi_launch")

Case = collections.namedtuple("Case", "name cls dtype channels_first C H W B in_off out_off explicit_last rows")


def _case(cls, dtype, cf, C, H, W, B=72, in_off=0, out_off=0, explicit_last=False, rows=False):
    name = f"{cls}-{np.dtype(dtype).name}-{'cf' if cf else 'cl'}-{C}x{H}x{W}-b{B}-i{in_off}-o{out_off}" + ("-rows" if rows else "")
    return Case(name, cls, np.dtype(dtype), cf, C, H, W, B, in_off, out_off, explicit_last, rows)


def _table():
    out = []
    for dtype in (np.uint8, np.float32):
        mis = 1 if dtype == np.uint8 else 4          # a float32 input stays a float32 pointer: 4-byte aligned
        # channels first: P = C planes of H rows of R = W elements, the right-hand tap S = 1 on
        out += [_case("staged_single", dtype, True, 3, 48, 80),                 # 3840 elements: one short chunk
                _case("staged_single", dtype, True, 2, 64, 64),                 # 4096: exactly one
                _case("staged_whole", dtype, True, 1, 128, 128, rows=True),     # 4 whole chunks; with and without a row table
                _case("staged_ragged", dtype, True, 6, 72, 72),                 # 5184 = 4096 + 1088
                _case("staged_single", dtype, True, 2, 100, 36),                # 3600: one short chunk of 100 rows of 36
                _case("elem_plane", dtype, True, 2, 9, 6, rows=True),           # 54 elements: no multiple of 4
                _case("elem_plane", dtype, True, 1, 70, 99),                    # 6930: two chunks on the per-element path
                _case("elem_in", dtype, True, 2, 72, 72, in_off=mis),
                _case("elem_in", dtype, True, 3, 64, 64, in_off=8),
                _case("elem_out", dtype, True, 6, 72, 72, out_off=4),
                _case("elem_out", dtype, True, 1, 64, 64, out_off=8),
                _case("elem_row", dtype, True, 1, 3, 8192, B=64),               # R + S = 8193
                _case("multi_launch", dtype, True, 1 << 17, 2, 2, B=96, explicit_last=True)]   # 2^17 workgroups a sample: 64 samples a launch
        # channels last: one plane of H rows of R = W C elements, the right-hand tap S = C on
        out += [_case("staged_single", dtype, False, 1, 64, 64),
                _case("staged_single", dtype, False, 6, 16, 16),                # 1536
                _case("staged_whole", dtype, False, 2, 128, 128, rows=True),    # 8 whole chunks
                _case("staged_whole", dtype, False, 1, 128, 128),
                _case("staged_ragged", dtype, False, 3, 48, 80),                # 11520 = 2 x 4096 + 3328
                _case("staged_ragged", dtype, False, 6, 96, 96),                # 55296 = 13 x 4096 + 2048: the visuotactile visual key
                _case("staged_ragged", dtype, False, 1, 72, 72),
                _case("staged_ragged", dtype, False, 2, 8, 4095, B=64),         # R + S = 8192 exactly: the longest staged row, the largest LDS
                _case("elem_plane", dtype, False, 3, 9, 6, rows=True),          # 162 elements
                _case("elem_plane", dtype, False, 1, 7, 10),                    # 70
                _case("elem_in", dtype, False, 6, 100, 36, in_off=mis),
                _case("elem_in", dtype, False, 2, 64, 64, in_off=12),
                _case("elem_out", dtype, False, 1, 72, 72, out_off=4),
                _case("elem_out", dtype, False, 3, 48, 80, out_off=12),
                _case("elem_row", dtype, False, 6, 3, 1366, B=64),              # R + S = 8202
                _case("elem_row", dtype, False, 1, 4, 8192, B=64),              # R + S = 8193
                _case("multi_launch", dtype, False, 1, 2, 2, B=MAX_BLOCKS + 96, explicit_last=True)]   # one workgroup a sample
    return out


CASES = _table()
# Cases of millions of tiny samples: their reference is augment_ref.warp_f32_batched (held to warp_f32 bit for bit on every other case).
def is_huge(case):
    return case.B > 100000


def _lowbit(n):
    return n & -n


def explicit_rows(H, W):
    """{shift class: float32 rows (apply, tx, ty)} that every case carries.  tx, ty are kornia's pixel translations; the shift the kernel
    applies is s = t n / (n - 1), so t = (n - 1) / 2^k gives s = n / 2^k exactly: an integer or an exact half."""
    inf, nan, big = np.inf, np.nan, 1e30
    hx, hy = W / 2 + 0.3, H / 2 + 0.45
    ex = (W - 1) / _lowbit(W) if W % 2 == 0 else 0.0      # s = the odd part of W, an exact integer below W
    ey = (H - 1) / _lowbit(H) if H % 2 == 0 else 0.0
    hfx = (W - 1) / (2 * _lowbit(W)) if W % 2 == 0 else (W - 1) / 2    # s = half an odd number, an exact half
    hfy = (H - 1) / (2 * _lowbit(H)) if H % 2 == 0 else (H - 1) / 2
    rows = {
        "zero": [(1, 0, 0)],
        "n_minus_1": [(1, W - 1, 0), (1, -(W - 1), 0), (1, 0, H - 1), (1, 0, -(H - 1)), (1, W - 1, -(H - 1))],
        "n": [(1, W, 0), (1, -W, 0), (1, 0, H), (1, 0, -H), (1, -W, H)],
        "half_fractional": [(1, hx, 0.25), (1, -hx, -0.6), (1, 0.7, hy), (1, -0.2, -hy), (1, hx, -hy), (1, -hx, hy)],
        "n_plus_5": [(1, W + 5, 0.5), (1, -(W + 5), 0.5), (1, 0.5, H + 5), (1, 0.5, -(H + 5)), (1, -(W + 5), H + 5)],
        "huge": [(1, big, 0), (1, -big, 1.5), (1, 0, big), (1, 1.5, -big)],
        "non_finite": [(1, inf, 0), (1, -inf, 0), (1, 0, inf), (1, 0, -inf), (1, nan, 0), (1, 0, nan), (1, nan, nan), (1, inf, -inf)],
        "integer": [(1, 3, -2), (1, -1, 1), (1, ex, 0), (1, 0, ey), (1, -ex, -ey), (1, ex, ey), (1, (W - 1) / 2, 0), (1, 0, -(H - 1) / 2)],
        "half": [(1, 2.5, -1.5), (1, -0.5, 0.5), (1, hfx, hfy), (1, -hfx, hfy)],
        "unapplied_huge": [(0, big, -inf), (0, nan, big), (0, W / 2, H / 2)],
    }
    return {k: np.array(v, np.float32).reshape(-1, 3) for k, v in rows.items()}


SHIFT_CLASSES = tuple(explicit_rows(8, 8))
DRAW = dict(translate=(1.0, 1.0), p=0.5)      # the draws that fill the rest of a case's rows (and the kernel's own, when it draws)


def case_seed(case):
    return 1000 + CASES.index(case)


def case_params(case):
    """float32 [B, 3]: the explicit rows of every shift class, then (explicit_last: preceded by) draws of the case's own seed."""
    ex = np.concatenate(list(explicit_rows(case.H, case.W).values()))
    drawn = draw_params(case_seed(case), 3, case.B - len(ex), DRAW["translate"], DRAW["p"], case.H, case.W)
    return np.ascontiguousarray(np.concatenate([drawn, ex] if case.explicit_last else [ex, drawn]), np.float32)


def explicit_slice(case, cls):
    """The rows of case_params(case) that are shift class cls."""
    ex = explicit_rows(case.H, case.W)
    start = case.B - sum(len(v) for v in ex.values()) if case.explicit_last else 0
    for k, v in ex.items():
        if k == cls:
            return slice(start, start + len(v))
        start += len(v)
    raise KeyError(cls)


DATA_KINDS = {np.dtype(np.uint8): ("u8",), np.dtype(np.float32): ("unit255", "signed_wide")}


def case_input(case, kind, n_samples=None):
    """The input batch of a case ([B, C, H, W] or [B, H, W, C]; n_samples: another number of samples, for a row table's source).
    u8: uniform bytes.  unit255: float32 uniform in [0, 255).  signed_wide: signed float32 with magnitudes 2^-20 .. 2^20, neighbours unrelated."""
    rng = np.random.default_rng(case_seed(case) * 7 + len(kind))
    B = case.B if n_samples is None else n_samples
    shape = (B, case.C, case.H, case.W) if case.channels_first else (B, case.H, case.W, case.C)
    if kind == "u8":
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    if kind == "unit255":
        return rng.random(shape, dtype=np.float32) * np.float32(255)
    assert kind == "signed_wide"
    mant = rng.random(shape, dtype=np.float32) + np.float32(1)
    expo = rng.integers(-20, 20, size=shape, dtype=np.int8)
    sign = rng.integers(0, 2, size=shape, dtype=np.int8) * np.int8(2) - np.int8(1)
    return np.ldexp(mant, expo).astype(np.float32) * sign.astype(np.float32)


def row_table(case, n_src):
    """int64 [B] source samples of a row-table run over n_src > B source samples: the last source sample (twice), then descending order with
    every seventh entry repeated."""
    rows = [n_src - 1, n_src - 1]
    r = n_src - 2
    while len(rows) < case.B:
        rows.append(r)
        if len(rows) % 7 == 0 and len(rows) < case.B:
            rows.append(r)
        r = r - 1 if r > 0 else n_src - 1
    return np.array(rows, np.int64)
