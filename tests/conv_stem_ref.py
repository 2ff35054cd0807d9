"""float64 numpy restatement of the device conv stem (tactile_gym_amd.torch_layers; csrc/tg_conv_stem.hip) and the error bounds
and exact-arithmetic cases its tests use.

forward / backward evaluate the layer's formulas in float64 with the exact product x * scale: no float32 step anywhere.

Bounds.  A float32 sum of n products, fused or not, in ANY order, differs from the exact sum by at most n u sum|a_i b_i| (1 + O(n u)) with
u = 2^-24 (each of the at most 2 n roundings is relative to a partial sum that sum|a_i b_i| bounds); the epilogue adds two roundings of
values bounded by scale sum|x w| + |b|.  With 2^-23 = 2 u in place of u, and K + 4 for K, the O(n u) terms are covered for every n here:
    fwd_bound = (K + 4) 2^-23 (scale sum_k |x_k| |w_k| + |b|)             per output element
    bwd_bound = (M + 4) 2^-23 scale sum |g| |x|,  M = B OH OW               per weight; dbias: the same with x = 1, scale = 1
They are derived, not measured.

Grid cases.  With integer x (uint8 values), integer w in [-64, 64], integer b, scale = 2^-8 and integer g in [-4, 4], every partial sum of
every order is an integer below 2^24 in magnitude (K <= 768: 768 * 255 * 64 < 2^24; M gmax 255 < 2^24 with g in [-gmax, gmax], which
grid_backward_case asserts: M <= 16448 at gmax = 4, M <= 21930 at gmax = 3), so float32
arithmetic is exact and the float64 result, rounded to float32, is the ONLY correct answer: the kernels must give those bits.  The weights
and gradients are drawn at random: a pattern symmetric in two indices would hide a row <-> column swap of an MFMA operand or result."""
import numpy as np

KERNEL, STRIDE, OUT = 8, 4, 32
f32, f64 = np.float32, np.float64
U8_SCALE = f32(1.0) / f32(255.0)
GRID_SCALE = f32(2.0 ** -8)

# (H, W, Cn, B, channels_first, x_is_float): the forward cases of tests/test_gpu_conv_stem_abi.py (and of the restatement's own check against
# torch).  (8, 8): one output; (40, 52): non-square, both layouts; Cn = 12; B = 65; (128, 128): 961 = 30 * 32 + 1 output positions;
# W = 530: 131 output columns, more than one column chunk of 128
FWD_CASES = [
    (8, 8, 1, 1, True, False), (8, 8, 12, 65, False, True), (8, 8, 3, 3, False, False), (8, 8, 2, 1, True, True),
    (11, 12, 2, 3, True, False), (11, 12, 6, 1, False, True),
    (36, 36, 3, 3, True, True), (36, 36, 1, 65, False, False),
    (37, 39, 6, 1, True, False), (37, 39, 2, 3, False, True),
    (40, 52, 3, 3, True, False), (40, 52, 3, 3, False, False), (40, 52, 12, 1, True, True), (40, 52, 12, 1, False, True),
    (128, 128, 1, 3, True, False), (128, 128, 1, 65, True, False), (128, 128, 2, 1, False, False), (128, 128, 3, 1, False, True),
    (128, 128, 12, 1, True, False),
    (8, 530, 1, 1, True, False), (12, 530, 2, 2, False, False),
]
# (H, W, Cn, B, channels_first, x_is_float): the backward cases
BWD_CASES = [
    (8, 8, 1, 1, True, False), (8, 8, 3, 5, False, False), (8, 8, 3, 3, True, True),
    (40, 52, 1, 3, False, False), (40, 52, 3, 5, True, False), (40, 52, 3, 1, False, True),
    (128, 128, 1, 5, True, False), (128, 128, 3, 3, False, False), (128, 128, 1, 1, True, True),
    # more regions than the 256 workgroups of a channel, so a workgroup walks on: its barrier between regions, its accumulator tile and its
    # bias sum carried over
    (8, 8, 2, 257, True, False),              # 257 regions of one position: workgroup 0 walks two
    (12, 12, 1, 600, False, False),           # 600 regions of 4 positions: workgroups walk 2 or 3; the second MFMA phase stays idle
    (16, 176, 1, 129, True, False),           # OW = 43, R = 2: strips of 2 rows and of 1 row; 258 regions; M = 16641
    (8, 530, 1, 129, False, True),            # OW = 131: chunks of 128 and 3; 258 regions; float32 NHWC; M = 16899
    (12, 530, 2, 3, True, False),             # chunks x strips without a wrap; two channels
]
# the gradient range of a backward grid case: two regions an image mean more than 128 positions an image, so a wrap with several strips or
# chunks needs M > 16448 and a narrower range
GMAX = {(16, 176, 1, 129, True, False): 3, (8, 530, 1, 129, False, True): 3}
POS, BWD_GROUPS = 128, 256                           # kStemPos, kStemBwdGroups


def gmax_of(case):
    return GMAX.get(tuple(case), 4)


def geometry(B, H, W):
    """stem_geom and stem_groups of csrc/tg_conv_stem.hip: how the OH x OW output positions of an image are cut into regions of at most 128
    (column chunks of Cw, strips of R rows) and how many workgroups a channel's backward pass runs."""
    OH, OW = out_hw(H, W)
    Cw = min(OW, POS)
    n_chunks = (OW + Cw - 1) // Cw
    R = min(POS // Cw, OH)
    n_strips = (OH + R - 1) // R
    regions = B * n_strips * n_chunks
    return dict(OH=OH, OW=OW, Cw=Cw, n_chunks=n_chunks, R=R, n_strips=n_strips, regions=regions, G=min(regions, BWD_GROUPS))


def region(geom, index):
    """stem_region: (image, first row, first column, rows, columns) of region `index`."""
    chunk, rest = index % geom["n_chunks"], index // geom["n_chunks"]
    strip, b = rest % geom["n_strips"], rest // geom["n_strips"]
    oy0, ox0 = strip * geom["R"], chunk * geom["Cw"]
    return b, oy0, ox0, min(geom["OH"] - oy0, geom["R"]), min(geom["OW"] - ox0, geom["Cw"])


def out_hw(H, W):
    return (H - KERNEL) // STRIDE + 1, (W - KERNEL) // STRIDE + 1


def x_shape(B, Cn, H, W, channels_first):
    return (B, Cn, H, W) if channels_first else (B, H, W, Cn)


def patches(x, channels_first):
    """float64 [B, OH, OW, K] of the input elements each output position reads, k = (c 8 + ky) 8 + kx."""
    x = np.asarray(x)
    x = np.ascontiguousarray((x if channels_first else x.transpose(0, 3, 1, 2)).astype(f64))
    B, Cn, H, W = x.shape
    OH, OW = out_hw(H, W)
    s = x.strides
    v = np.lib.stride_tricks.as_strided(x, (B, OH, OW, Cn, KERNEL, KERNEL), (s[0], STRIDE * s[2], STRIDE * s[3], s[1], s[2], s[3]))
    return v.reshape(B, OH, OW, Cn * KERNEL * KERNEL)


def forward(x, w, b, scale, channels_first):
    """(y, fwd_bound): float64 [B, 32, OH, OW] each."""
    P = patches(x, channels_first)
    w2 = np.asarray(w, f64).reshape(OUT, -1)
    b = np.asarray(b, f64)
    s = f64(scale)
    y = np.maximum(s * (P @ w2.T) + b, 0.0)
    K = w2.shape[1]
    bound = (K + 4) * 2.0 ** -23 * (s * (np.abs(P) @ np.abs(w2).T) + np.abs(b))
    return y.transpose(0, 3, 1, 2), bound.transpose(0, 3, 1, 2)


def backward(x, y, dy, scale, channels_first):
    """(dweight [32, Cn, 8, 8], dbias [32], bwd_bound of dweight, of dbias) in float64, from the forward's output y (only y > 0 is used)."""
    P = patches(x, channels_first)
    B, OH, OW, K = P.shape
    g = np.where(np.asarray(y) > 0, np.asarray(dy, f64), 0.0).transpose(0, 2, 3, 1).reshape(B * OH * OW, OUT)
    P = P.reshape(B * OH * OW, K)
    s, M = f64(scale), B * OH * OW
    dw = s * (g.T @ P)
    db = g.sum(axis=0)
    shape = (OUT, K // 64, KERNEL, KERNEL)
    return (dw.reshape(shape), db, ((M + 4) * 2.0 ** -23 * s * (np.abs(g).T @ np.abs(P))).reshape(shape),
            (M + 4) * 2.0 ** -23 * np.abs(g).sum(axis=0))


def _images(rng, B, Cn, H, W, channels_first, x_is_float):
    x = rng.integers(0, 256, x_shape(B, Cn, H, W, channels_first), dtype=np.uint8)
    return x.astype(f32) if x_is_float else x


def grid_forward_case(rng, B, Cn, H, W, channels_first, x_is_float):
    """(x, w, b, scale) on which float32 arithmetic is exact in every order."""
    assert Cn * 64 <= 768
    w = rng.integers(-64, 65, (OUT, Cn, KERNEL, KERNEL)).astype(f32)
    b = rng.integers(-100, 101, (OUT,)).astype(f32)
    return _images(rng, B, Cn, H, W, channels_first, x_is_float), w, b, GRID_SCALE


def random_forward_case(rng, B, Cn, H, W, channels_first, x_is_float):
    w = (0.05 * rng.standard_normal((OUT, Cn, KERNEL, KERNEL))).astype(f32)
    b = (0.05 * rng.standard_normal((OUT,))).astype(f32)
    return _images(rng, B, Cn, H, W, channels_first, x_is_float), w, b, U8_SCALE


def grid_backward_case(rng, B, Cn, H, W, channels_first, x_is_float, gmax=4):
    """(x, y, dy, scale): y has zeros (about half), so the mask matters; dy is an integer in [-gmax, gmax] everywhere."""
    OH, OW = out_hw(H, W)
    assert B * OH * OW * gmax * 255 < 2 ** 24                             # every partial sum of every order is an integer float32 holds
    y = np.maximum(rng.integers(-3, 4, (B, OUT, OH, OW)), 0).astype(f32)
    dy = rng.integers(-gmax, gmax + 1, (B, OUT, OH, OW)).astype(f32)
    return _images(rng, B, Cn, H, W, channels_first, x_is_float), y, dy, GRID_SCALE


def random_backward_case(rng, B, Cn, H, W, channels_first, x_is_float):
    OH, OW = out_hw(H, W)
    y = np.maximum(rng.standard_normal((B, OUT, OH, OW)), 0).astype(f32)
    dy = rng.standard_normal((B, OUT, OH, OW)).astype(f32)
    return _images(rng, B, Cn, H, W, channels_first, x_is_float), y, dy, U8_SCALE
