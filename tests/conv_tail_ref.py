"""float64 numpy restatement of the device NatureCNN tail (tactile_gym_amd.torch_layers.conv_relu / linear_relu; csrc/tg_conv.hip; DESIGN.md
4.21) - a valid strided convolution with bias and ReLU, its dweight, dbias and dx - and the error bounds, cases, exact-arithmetic generators
and order probes its tests use.

forward / backward evaluate the layer's formulas in float64: no float32 step anywhere.

Bounds.  The derivation of conv_stem_ref's docstring: a float32 sum of n products, fused or not, in ANY order, differs from the exact sum by
at most n u sum|a_i b_i| (1 + O(n u)), u = 2^-24; with 2^-23 = 2 u for u and n + 4 for n the O(n u) terms and the epilogue's rounding are
covered for every n here:
    fwd      (K + 4) 2^-23 (sum_k |x_k| |w_k| + |b|)          per output element, K = Cin KH KW
    dweight  (M + 4) 2^-23 sum_m |g| |x|                      per weight, M = B OH OW
    dbias    (M + 4) 2^-23 sum_m |g|
    dx       (J + 4) 2^-23 sum_j |g| |w|                      per input element, J = Cout KH KW
They are derived, not measured.

Grid cases.  Integer x in [0, 15], integer w in [-8, 8], integer b, integer g in [-4, 4]: every partial sum of every order is an integer below
2^24 in magnitude (the generators assert K 15 8, M 4 15 and J 4 8 < 2^24), so float32 arithmetic is exact and the float64 result, rounded to
float32, is the ONLY correct answer: the kernels must give those bits.  The values are drawn at random: a pattern symmetric in two indices
would hide a row <-> column swap of an MFMA operand or result.

Order probes.  All products of an element's chain are zero but three: +2^24, +1, -2^24 at chosen chain positions p1 < p2 < p3 (built as
2^12 * 2^12, 1 * 1, 2^12 * -2^12).  The ascending chain gives ((2^24 + 1) - 2^24) = 0 exactly, since 2^24 + 1 rounds to 2^24; the reversed
order, a pairwise order ((p1 + p3) + p2) and a split between the first two (p1 + (p2 + p3)) all give 1.  The kernels have ONE chain per
element (K is not cut into segments), so there is no segment boundary to probe."""
import numpy as np

f32, f64 = np.float32, np.float64

# (Cin, H, W, Cout, KH, KW, stride, B)
CASES = [
    (2, 3, 3, 32, 3, 3, 1, 1),                       # one output position, one tile, K = 18 (a chunk shorter than 32)
    (32, 6, 6, 64, 4, 4, 2, 9),                      # 4 positions per image: a tile spans 8 images, the second tile holds 4 valid positions
    (32, 8, 8, 64, 4, 4, 2, 3), (32, 8, 8, 64, 4, 4, 2, 65),          # conv2, conv3 and the linear layer of the 36 x 36 observation
    (64, 3, 3, 64, 3, 3, 1, 3), (64, 3, 3, 64, 3, 3, 1, 65),
    (64, 1, 1, 32, 1, 1, 1, 3), (64, 1, 1, 32, 1, 1, 1, 65),
    (32, 31, 31, 64, 4, 4, 2, 1), (32, 31, 31, 64, 4, 4, 2, 3),       # conv2 of 128 x 128: 196 positions = 6 tiles + 4; image boundaries inside tiles
    (64, 14, 14, 64, 3, 3, 1, 1), (64, 14, 14, 64, 3, 3, 1, 3),       # conv3 of 128 x 128
    (64, 12, 12, 512, 12, 12, 1, 1), (64, 12, 12, 512, 12, 12, 1, 33), (64, 12, 12, 512, 12, 12, 1, 65),   # the real linear: K = 9216, 16 channel tiles
    (4, 10, 13, 96, 3, 2, 3, 5),                     # non-square input and kernel, stride 3, three channel tiles; unread input rows and columns
    # backward walk: the number of partials is P = min(ceil(M / 256), 64, ...) and workgroup p walks the 64-position chunks p, p + P, ...: with
    # M = 800 * 16 = 12800 there are 200 chunks and P = 50, so every workgroup walks FOUR chunks and carries its accumulator tile and bias sum
    (2, 5, 5, 32, 2, 2, 1, 800),
    (2, 3, 3, 32, 2, 2, 1, 4200),                    # M = 16800: 263 chunks over P = 64 workgroups (the cap): walks of 4 and 5 chunks
]
# The paths of csrc/tg_conv.hip that CASES leaves unrun (`route` names them; tests/test_gpu_conv_tail_paths.py runs them)
PATH_CASES = [
    (32, 8, 8, 128, 4, 4, 2, 3),                     # k_conv_fwd's four-channel-tile wave layout (Cout >= 128), one channel block; K = 512, M = 27
    (5, 9, 9, 160, 4, 4, 1, 15),                     # two such channel blocks, the second with one live tile; K = 80: chunks 32, 32, 16 and K % 64 = 16;
                                                     # M = 540: P = 3 partials over three channel blocks and two k blocks
    (40, 6, 6, 32, 3, 3, 1, 5),                      # K = 360: a last chunk of 8, K % 64 = 40; Cin = 40: k_conv_dx's second channel tile is partly valid
    (2, 17, 18, 32, 16, 16, 1, 2),                   # a 16 x 16 kernel: ky / stride up to 15 in dx's packed table; J = 8192, most dx MFMAs skipped
    (2, 23, 21, 64, 7, 6, 4, 3),                     # stride 4: ky % stride = 3; K = 84; non-square, three unread input columns
    (64, 3, 3, 64, 3, 3, 3, 3),                      # the linear pair at stride 3 (H == KH decides, not the stride)
    (6, 3, 3, 32, 3, 3, 1, 33),                      # K = 54: the generic forward, k_conv_lin_dx with 22 valid k in its second tile, two batch tiles
    (2, 5, 5, 32, 2, 2, 1, 8),                       # M = 128 exactly: one full 128-position block, two full backward chunks
]
CAP_CASE = (64, 16, 16, 512, 16, 16, 1, 1025)        # the smallest shape at which 2^25 / (Cout K) = 4 binds P (ceil(M / 256) = 5): walks of 5, 4, 4, 4 chunks
REAL_128 = [(32, 31, 31, 64, 4, 4, 2), (64, 14, 14, 64, 3, 3, 1), (64, 12, 12, 512, 12, 12, 1)]   # the three real shapes (batch invariance)
BWD_SHARE, BWD_CHUNK, BWD_MAX_PARTS, BWD_MAX_FLOATS, BIAS_PARTS = 256, 64, 64, 1 << 25, 4        # csrc/tg_conv.hip's constants


def parts(M, Cout, K):
    """conv_parts of csrc/tg_conv.hip: the number of dweight partials."""
    return max(1, min(-(-M // BWD_SHARE), BWD_MAX_PARTS, BWD_MAX_FLOATS // (Cout * K)))


def workspace_bytes(case):
    Cin, H, W, Cout, KH, KW, stride, B = case
    OH, OW = out_hw(H, W, KH, KW, stride)
    K = Cin * KH * KW
    return 4 * parts(B * OH * OW, Cout, K) * (Cout * K + BIAS_PARTS * Cout)


def route(case, aligned=True):
    """The launchers' decisions for one case (tg_conv_relu and tg_conv_relu_bwd of csrc/tg_conv.hip, restated): which kernels run and which of
    their branches the sizes reach.  `aligned`: whether x and w are 16-byte aligned.  Entries that belong to a kernel that does not run are None."""
    Cin, H, W, Cout, KH, KW, stride, B = case
    OH, OW = out_hw(H, W, KH, KW, stride)
    K, M = Cin * KH * KW, B * OH * OW
    linear = H == KH and W == KW
    r = dict(K=K, M=M, stride=stride)
    r["fwd"] = "lin" if linear and K % 32 == 0 and aligned else "generic"
    generic = r["fwd"] == "generic"
    cl = 2 if Cout >= 128 else (1 if Cout >= 64 else 0)
    CW = 32 << cl
    r["fwd_cl"] = cl if generic else None
    r["fwd_cblocks"] = -(-Cout // CW) if generic else None
    r["fwd_last_cblock_partial"] = Cout % CW != 0 if generic else None
    r["fwd_chunks"] = [32] * (K // 32) + ([K % 32] if K % 32 else []) if generic else None
    r["n_kblocks"] = -(-K // 64)
    r["k_mod_64"] = "0" if K % 64 == 0 else ("1..32" if K % 64 <= 32 else "33..63")
    r["n_cblocks"] = -(-Cout // 64)
    r["P"] = parts(M, Cout, K)
    r["cap_bound"] = BWD_MAX_FLOATS // (Cout * K) < min(-(-M // BWD_SHARE), BWD_MAX_PARTS)
    r["walks"] = sorted({len(range(p, -(-M // BWD_CHUNK), r["P"])) for p in range(r["P"])}, reverse=True)
    r["dx"] = "lin" if linear else "generic"
    r["dx_cl"] = (1 if Cin > 32 else 0) if not linear else None
    r["dx_last_ctile_partial"] = Cin % 32 != 0 if not linear else None
    r["dx_max_ky_div"] = max((KH - 1) // stride, (KW - 1) // stride) if not linear else None      # the 4-bit fields of k_conv_dx's table
    r["dx_max_ky_mod"] = min(max(KH, KW) - 1, stride - 1) if not linear else None                   # the 2-bit fields
    r["lin_dx_last_ktile"] = K % 32 if linear else None                                              # valid k of k_conv_lin_dx's last tile (0: full)
    r["batch_tiles"] = -(-B // 32) if linear else None
    return r


def case_id(case):
    Cin, H, W, Cout, KH, KW, stride, B = case
    return f"c{Cin}-{H}x{W}-o{Cout}-k{KH}x{KW}-s{stride}-b{B}"


def out_hw(H, W, KH, KW, stride):
    return (H - KH) // stride + 1, (W - KW) // stride + 1


def patches(x, KH, KW, stride):
    """float64 [B, OH, OW, K] of the input elements each output position reads, k = (c KH + ky) KW + kx."""
    x = np.ascontiguousarray(np.asarray(x).astype(f64))
    B, Cin, H, W = x.shape
    OH, OW = out_hw(H, W, KH, KW, stride)
    s = x.strides
    v = np.lib.stride_tricks.as_strided(x, (B, OH, OW, Cin, KH, KW), (s[0], stride * s[2], stride * s[3], s[1], s[2], s[3]))
    return v.reshape(B, OH, OW, Cin * KH * KW)


def forward(x, w, b, stride):
    """(y, fwd_bound): float64 [B, Cout, OH, OW] each."""
    Cout, _, KH, KW = w.shape
    P = patches(x, KH, KW, stride)
    w2, b = np.asarray(w, f64).reshape(Cout, -1), np.asarray(b, f64)
    y = np.maximum(P @ w2.T + b, 0.0)
    K = w2.shape[1]
    bound = (K + 4) * 2.0 ** -23 * (np.abs(P) @ np.abs(w2).T + np.abs(b))
    return y.transpose(0, 3, 1, 2), bound.transpose(0, 3, 1, 2)


def _scatter(dP, shape, KH, KW, stride):
    """The transpose of `patches`: dP [B, OH, OW, Cin, KH, KW] added into an input-shaped array."""
    B, Cin, H, W = shape
    OH, OW = dP.shape[1:3]
    dx = np.zeros(shape, f64)
    for ky in range(KH):
        for kx in range(KW):
            dx[:, :, ky:ky + stride * (OH - 1) + 1:stride, kx:kx + stride * (OW - 1) + 1:stride] += dP[:, :, :, :, ky, kx].transpose(0, 3, 1, 2)
    return dx


def backward(x, w, y, dy, stride):
    """dict(dw, db, dx, dw_bound, db_bound, dx_bound) in float64, from the forward's output y (only y > 0 is used)."""
    Cout, Cin, KH, KW = w.shape
    P = patches(x, KH, KW, stride)
    B, OH, OW, K = P.shape
    M, J = B * OH * OW, Cout * KH * KW
    g = np.where(np.asarray(y) > 0, np.asarray(dy, f64), 0.0).transpose(0, 2, 3, 1).reshape(M, Cout)
    P = P.reshape(M, K)
    w2 = np.asarray(w, f64).reshape(Cout, K)
    u = 2.0 ** -23
    shape6 = (B, OH, OW, Cin, KH, KW)
    return dict(dw=(g.T @ P).reshape(w.shape), db=g.sum(axis=0), dx=_scatter((g @ w2).reshape(shape6), x.shape, KH, KW, stride),
                dw_bound=((M + 4) * u * (np.abs(g).T @ np.abs(P))).reshape(w.shape), db_bound=(M + 4) * u * np.abs(g).sum(axis=0),
                dx_bound=(J + 4) * u * _scatter((np.abs(g) @ np.abs(w2)).reshape(shape6), x.shape, KH, KW, stride))


def dweight_dbias(x, w, y, dy, stride):
    """(dw, db) of `backward` alone, for a case too large to form dx and the bounds on the host."""
    P = patches(x, w.shape[2], w.shape[3], stride)
    g = np.where(np.asarray(y) > 0, np.asarray(dy, f64), 0.0).transpose(0, 2, 3, 1).reshape(-1, w.shape[0])
    return (g.T @ P.reshape(g.shape[0], -1)).reshape(w.shape), g.sum(axis=0)


def unread(case):
    """bool [H, W]: the input rows and columns that no output position reads (their dx is 0)."""
    Cin, H, W, Cout, KH, KW, stride, B = case
    OH, OW = out_hw(H, W, KH, KW, stride)
    m = np.ones((H, W), bool)
    m[:stride * (OH - 1) + KH, :stride * (OW - 1) + KW] = False
    return m


def grid_case(rng, case):
    """(x, w, b, y, dy) on which float32 arithmetic is exact in every order; y (the backward's mask, about half zeros) and dy are free inputs."""
    Cin, H, W, Cout, KH, KW, stride, B = case
    OH, OW = out_hw(H, W, KH, KW, stride)
    K, J, M = Cin * KH * KW, Cout * KH * KW, B * OH * OW
    assert K * 15 * 8 < 2 ** 24 and M * 4 * 15 < 2 ** 24 and J * 4 * 8 < 2 ** 24      # every partial sum of every order is an integer float32 holds
    x = rng.integers(0, 16, (B, Cin, H, W)).astype(f32)
    w = rng.integers(-8, 9, (Cout, Cin, KH, KW)).astype(f32)
    b = rng.integers(-100, 101, (Cout,)).astype(f32)
    y = np.maximum(rng.integers(-3, 4, (B, Cout, OH, OW)), 0).astype(f32)
    dy = rng.integers(-4, 5, (B, Cout, OH, OW)).astype(f32)
    return x, w, b, y, dy


def random_case(rng, case):
    """(x, w, b, y, dy): w ~ 0.05 N, x ~ |N|."""
    Cin, H, W, Cout, KH, KW, stride, B = case
    OH, OW = out_hw(H, W, KH, KW, stride)
    x = np.abs(rng.standard_normal((B, Cin, H, W))).astype(f32)
    w = (0.05 * rng.standard_normal((Cout, Cin, KH, KW))).astype(f32)
    b = (0.05 * rng.standard_normal((Cout,))).astype(f32)
    y = np.maximum(rng.standard_normal((B, Cout, OH, OW)), 0).astype(f32)
    dy = rng.standard_normal((B, Cout, OH, OW)).astype(f32)
    return x, w, b, y, dy


# ---------------------------------------------------------------------------------------------------------------- order probes
BIG = f32(2.0 ** 12)
PROBE_A = (BIG, f32(1.0), BIG)                       # x (forward) or g (dx) at the three chain positions
PROBE_B = (BIG, f32(1.0), -BIG)                      # w


def probe_orders():
    """The three products summed in float32 in the orders named: dict(ascending=0, reversed=1, pairwise=1, split=1)."""
    p = [f32(a) * f32(b) for a, b in zip(PROBE_A, PROBE_B)]
    z = f32(0.0)
    return dict(ascending=f32(f32(f32(z + p[0]) + p[1]) + p[2]), reversed=f32(f32(f32(z + p[2]) + p[1]) + p[0]),
                pairwise=f32(f32(p[0] + p[2]) + p[1]), split=f32(f32(z + p[0]) + f32(f32(z + p[1]) + p[2])))


def _windows(n, step=1):
    return [(i, i + 1, i + 2) for i in range(0, n - 2, step)]


def forward_probe_sets():
    """[(shape (Cin, H, W, Cout, KH, KW, stride), [(k1, k2, k3), ...])]: chain positions of the forward probes.  K = 18 and K = 512: every window of
    three consecutive k, so the pair (k1, k2) and the pair (k2, k3) each fall inside one MFMA's two k and across two MFMAs, across every channel
    boundary and across the 32-k staging chunks.  The real linear (K = 9216): windows at the ends, at channel boundaries, at chunk boundaries,
    far-apart triples and random ones."""
    rng = np.random.default_rng(5)
    lin = [(0, 1, 2), (1, 2, 3), (142, 143, 144), (143, 144, 145), (30, 31, 32), (31, 32, 33), (4606, 4607, 4608), (4607, 4608, 4609),
           (9213, 9214, 9215), (9212, 9213, 9214), (0, 4608, 9215), (1, 4607, 9214), (0, 1, 9215), (0, 9214, 9215)]
    lin += [tuple(sorted(int(v) for v in rng.choice(9216, 3, replace=False))) for _ in range(50)]
    return [((2, 3, 3, 32, 3, 3, 1), _windows(18) + [(0, 8, 9), (8, 9, 17), (0, 16, 17)]),
            ((32, 8, 8, 64, 4, 4, 2), _windows(512)),
            ((64, 12, 12, 512, 12, 12, 1), lin)]


def path_forward_probe_sets():
    """As forward_probe_sets, on k_conv_fwd's chains with a short last chunk behind full ones: K = 80 (chunks 32, 32, 16; Cout = 160) and K = 360
    (a last chunk of 8).  Every window of three consecutive k: across the 31 / 32 and 63 / 64 chunk boundaries and into the short chunk."""
    return [((5, 9, 9, 160, 4, 4, 1), _windows(80)), ((40, 6, 6, 32, 3, 3, 1), _windows(360))]


def forward_probe(shape, triples):
    """(x, w, b, at): image i carries triple i in the window of output position at[i] = (oy, ox) against row co = i % Cout of w; y[i, i % Cout,
    oy, ox] must be exactly 0.  Consecutive images use different rows, so overlapping windows of k never meet in one row."""
    Cin, H, W, Cout, KH, KW, stride = shape
    OH, OW = out_hw(H, W, KH, KW, stride)
    B = len(triples)
    x, w, b = np.zeros((B, Cin, H, W), f32), np.zeros((Cout, Cin, KH, KW), f32), np.zeros((Cout,), f32)
    at = []
    seen = {}
    for i, tr in enumerate(triples):
        co, oy, ox = i % Cout, (i // 3) % OH, i % OW
        at.append((oy, ox))
        for k, xv, wv in zip(tr, PROBE_A, PROBE_B):
            c, ky, kx = k // (KH * KW), (k // KW) % KH, k % KW
            x[i, c, oy * stride + ky, ox * stride + kx] = xv
            assert seen.setdefault((co, k), wv) == wv                      # two triples of one row never disagree on a weight
            w[co, c, ky, kx] = wv
    return x, w, b, at


def dx_terms(shape, iy, ix):
    """The j = (co KH + ky) KW + kx, ascending, whose term exists for input position (iy, ix), with their (co, oy, ox, ky, kx)."""
    Cin, H, W, Cout, KH, KW, stride = shape
    OH, OW = out_hw(H, W, KH, KW, stride)
    out = []
    for co in range(Cout):
        for ky in range(KH):
            for kx in range(KW):
                dy_, dx_ = iy - ky, ix - kx
                if dy_ >= 0 and dx_ >= 0 and dy_ % stride == 0 and dx_ % stride == 0 and dy_ // stride < OH and dx_ // stride < OW:
                    out.append(((co * KH + ky) * KW + kx, co, dy_ // stride, dx_ // stride, ky, kx))
    return out


def dx_probe_sets():
    """[(shape, (iy, ix), n_windows)]: the dx probes take every window of three consecutive EXISTING terms of element (c, iy, ix).
    (4, 6, 6, 32, 3, 3, 1), (2, 2): all 288 j exist (in-pair and across-pair windows, across every co).  (32, 8, 8, 64, 4, 4, 2), (2, 2):
    stride 2, only ky, kx in {0, 2} exist: 256 of 1024 terms, each alone in its MFMA, most MFMAs skipped.  (64, 3, 3, 64, 3, 3, 1), (1, 2):
    OH = OW = 1, one term per co."""
    return [((4, 6, 6, 32, 3, 3, 1), (2, 2)), ((32, 8, 8, 64, 4, 4, 2), (2, 2)), ((64, 3, 3, 64, 3, 3, 1), (1, 2))]


def path_dx_probe_sets():
    """As dx_probe_sets, at the tops of the fields of k_conv_dx's packed table.  (4, 23, 21, 64, 7, 6, 4), (4, 4): stride 4, only ky, kx in {0, 4}
    exist: 256 terms, each alone in its MFMA.  (3, 17, 18, 32, 16, 16, 1), (15, 15): a 16 x 16 kernel, ky in {14, 15}, kx in {13, 14, 15}: 192
    terms with ky / stride of 14 and 15."""
    return [((4, 23, 21, 64, 7, 6, 4), (4, 4)), ((3, 17, 18, 32, 16, 16, 1), (15, 15))]


def dx_probe(shape, at):
    """(x, w, y, dy, n): image i carries window i of the existing terms of input element (c = i % Cin, iy, ix) in dy against w[:, c]; dx[i, i % Cin,
    iy, ix] must be exactly 0.  y = 1 everywhere (nothing is masked)."""
    Cin, H, W, Cout, KH, KW, stride = shape
    OH, OW = out_hw(H, W, KH, KW, stride)
    iy, ix = at
    terms = dx_terms(shape, iy, ix)
    wins = _windows(len(terms))
    B = len(wins)
    assert Cin >= 3                                                        # windows i and i + 1, i + 2 overlap: they need different columns c
    x, w = np.zeros((B, Cin, H, W), f32), np.zeros((Cout, Cin, KH, KW), f32)
    y, dy = np.ones((B, Cout, OH, OW), f32), np.zeros((B, Cout, OH, OW), f32)
    seen = {}
    for i, win in enumerate(wins):
        c = i % Cin
        for t, gv, wv in zip(win, PROBE_A, PROBE_B):
            j, co, oy, ox, ky, kx = terms[t]
            dy[i, co, oy, ox] = gv
            assert seen.setdefault((c, j), wv) == wv
            w[co, c, ky, kx] = wv
    return x, w, y, dy, B
