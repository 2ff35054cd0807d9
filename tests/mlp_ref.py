"""float64 numpy restatement of the device MLP towers (tactile_gym_amd.mlp; csrc/tg_mlp.hip), the error bounds and the
exact-arithmetic cases its tests use.

A tower is a list of layers dict(w [out, in], b [out], act, w2, b2): h_l = act(h_{l-1} w^T + b); w2 / b2 (None except on a last layer with two
row blocks) are further rows of the same layer whose outputs are kept apart.  The input is the pair (x0 [B, Ka], x1 [B, Kb] or None), standing
for the concatenation of its columns.

Bounds (derived, not measured).  A float32 sum of n products, fused or not, in ANY order, differs from the exact sum by at most
n u sum|a_i b_i| (1 + O(n u)), u = 2^-24; adding the bias is one more rounding.  With 2^-23 = 2 u for u and n + 4 for n:
    e_z = (in + 4) 2^-23 (sum_k |h_{l-1}| |w| + |b|)                        per element, from the previous layer's float32 bits
    e_h = e_z + 2^-23 |h|                                                    ReLU and Tanh are 1-Lipschitz; tanh is rounded once from double
Propagated through a tower (the outputs, from the input's bits): the previous layer's error E passes the layer as E |w|^T, and the layer's
own e_z is taken at |h| + E.  Backward, from the given h_l and dy:  g = dh act'(h) costs no rounding for none / ReLU and three for Tanh
(t = h h, u = 1 - t, g = dh u: at most 2^-23 |dh| (h^2 + 2 |1 - h^2|));  the sums over rows dbias = sum g, dweight = sum g h_{l-1} get
(B + 4) 2^-23 sum|.| plus the terms' own errors;  dh_{l-1} = g w gets (out + 4) 2^-23 |g| |w| plus e_g |w|;  dx, the towers' dh_0 added in
tower order, gets T 2^-23 sum_t |dh_0| more.

Exact cases.  Integer x, w in {-1, 0, 1} (sparse at wide layers), integer b, activations none / ReLU: `assert_exact` checks that every term is
an integer and that every sum of ABSOLUTE terms stays below 2^24, so every partial sum in every order is an integer float32 holds exactly and
the float64 result, rounded to float32, is the ONLY correct answer.  The draws are random, so asymmetric in every index: a swapped MFMA
operand or a transposed C/D map cannot pass.

The k tail.  The kernel finishes a chain whose length is odd, or no multiple of its 32-wide staging chunk, with the operand pair (-0.0, +0.0).
`tail_operands_keep_bits` shows that fmaf(-0.0, +0.0, acc) has acc's bits for every float32 acc, -0.0 included, and that the obvious pair
(0.0, 0.0) does not: fmaf(0, 0, -0.0) = +0.0."""
import numpy as np

f32, f64 = np.float32, np.float64
E = 2.0 ** -23
ACTS = ("none", "tanh", "relu")
EXACT_LIMIT = 2.0 ** 24


def layer(w, b, act="none", w2=None, b2=None):
    return dict(w=w, b=b, act=act, w2=w2, b2=b2)


def cat_input(x):
    x0, x1 = x
    return np.asarray(x0, f64) if x1 is None else np.concatenate([np.asarray(x0, f64), np.asarray(x1, f64)], axis=1)


def full_w(ly):
    """(w [out + out2, in], b [out + out2]) in float64: both row blocks."""
    w, b = np.asarray(ly["w"], f64), np.asarray(ly["b"], f64)
    if ly.get("w2") is not None:
        w, b = np.concatenate([w, np.asarray(ly["w2"], f64)]), np.concatenate([b, np.asarray(ly["b2"], f64)])
    return w, b


def act(z, name):
    return np.tanh(z) if name == "tanh" else np.maximum(z, 0.0) if name == "relu" else z


def dact(h, name):
    """act'(z) from h = act(z)."""
    return 1.0 - h * h if name == "tanh" else (h > 0).astype(f64) if name == "relu" else np.ones_like(h)


def layer_forward(hprev, ly, err_prev=None):
    """(h, bound) of one layer in float64 from hprev [B, in] (float32 bits, or exact values with their error bound err_prev)."""
    hprev = np.asarray(hprev, f64)
    w, b = full_w(ly)
    h = act(hprev @ w.T + b, ly["act"])
    mag = np.abs(hprev) if err_prev is None else np.abs(hprev) + err_prev
    e_z = (w.shape[1] + 4) * E * (mag @ np.abs(w).T + np.abs(b))
    if err_prev is not None:
        e_z = e_z + err_prev @ np.abs(w).T
    return h, e_z + E * (np.abs(h) + (e_z if err_prev is not None else 0.0))


def tower_forward(x, tower):
    """Per layer (h, propagated bound), float64 [B, out + out2] each, from the input's bits."""
    h, err, out = cat_input(x), None, []
    for ly in tower:
        h, err = layer_forward(h, ly, err if err is not None else np.zeros_like(h))
        out.append((h, err))
    return out


def tower_backward(x, tower, hs, dy):
    """From the given h_l (list of [B, out + out2], float32 bits) and dy [B, out + out2] of the last layer:
    (grads, bounds, dh0, dh0_bound); grads[l] = (dweight [out + out2, in], dbias [out + out2]), bounds[l] likewise."""
    B = np.asarray(dy).shape[0]
    dh, e_dh = np.asarray(dy, f64), np.zeros(np.asarray(dy).shape)
    grads, bounds = [None] * len(tower), [None] * len(tower)
    for l in range(len(tower) - 1, -1, -1):
        ly = tower[l]
        w, _ = full_w(ly)
        h = np.asarray(hs[l], f64)
        hprev = np.asarray(hs[l - 1], f64) if l else cat_input(x)
        d = dact(h, ly["act"])
        g = dh * d
        e_g = e_dh * np.abs(d)
        if ly["act"] == "tanh":
            e_g = e_g + E * (np.abs(dh) + e_dh) * (h * h + 2 * np.abs(d))
        grads[l] = (g.T @ hprev, g.sum(axis=0))
        bounds[l] = ((B + 4) * E * (np.abs(g).T @ np.abs(hprev)) + e_g.T @ np.abs(hprev), (B + 4) * E * np.abs(g).sum(axis=0) + e_g.sum(axis=0))
        dh_new = g @ w
        e_dh = (w.shape[0] + 4) * E * ((np.abs(g) + e_g) @ np.abs(w)) + e_g @ np.abs(w)
        dh = dh_new
    return grads, bounds, dh, e_dh


def sum_dx(dh0s, bounds):
    """dx = the towers' dh_0 added in tower order, and its bound."""
    total = sum(dh0s)
    return total, sum(bounds) + len(dh0s) * E * sum(np.abs(d) for d in dh0s)


# ---------------------------------------------------------------------------------------------------------------- the k tail
def _fma32(a, b, c):
    """fmaf on float32 values whose product is exactly representable in float64 and whose sum rounds once: float64 holds a * b + c of the
    operands used here (zeros, and c arbitrary) exactly."""
    with np.errstate(all="ignore"):
        return f32(f64(a) * f64(b) + f64(c))


def tail_operands_keep_bits():
    """True when fmaf(-0.0, +0.0, acc) keeps acc's bits for a set of float32 values that covers both zeros, subnormals, the extremes,
    infinities and a NaN - and fmaf(+0.0, +0.0, -0.0) does not keep them."""
    accs = np.array([0.0, -0.0, 1e-45, -1e-45, 1.17549435e-38, 1.0, -1.0, 3.4028235e38, -3.4028235e38, np.inf, -np.inf, np.nan,
                     0.1, -7.25, 16777216.0], dtype=f32)
    kept = all(_fma32(f32(-0.0), f32(0.0), c).view(np.uint32) == c.view(np.uint32) or (np.isnan(c) and np.isnan(_fma32(f32(-0.0), f32(0.0), c)))
               for c in accs)
    naive = _fma32(f32(0.0), f32(0.0), f32(-0.0))
    return bool(kept) and naive.view(np.uint32) == f32(0.0).view(np.uint32) and naive.view(np.uint32) != f32(-0.0).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- cases
def random_tower(rng, K0, widths, acts, two=0):
    """N(0, 0.05) weights and biases; two > 0: the last layer gets a second block of `two` rows."""
    tower, width = [], K0
    for i, (out, a) in enumerate(zip(widths, acts)):
        ly = layer((0.05 * rng.standard_normal((out, width))).astype(f32), (0.05 * rng.standard_normal(out)).astype(f32), a)
        if two and i == len(widths) - 1:
            ly["w2"], ly["b2"] = (0.05 * rng.standard_normal((two, width))).astype(f32), (0.05 * rng.standard_normal(two)).astype(f32)
        tower.append(ly)
        width = out
    return tower


def _sparse_w(rng, out, width):
    """{-1, 0, 1}, about 8 non-zeros a row at wide layers."""
    keep = rng.random((out, width)) < min(1.0, 8.0 / width)
    return (rng.integers(0, 2, (out, width)) * 2 - 1).astype(f32) * keep


def exact_tower(rng, K0, widths, acts, two=0):
    assert all(a in ("none", "relu") for a in acts)
    tower, width = [], K0
    for i, (out, a) in enumerate(zip(widths, acts)):
        ly = layer(_sparse_w(rng, out, width), rng.integers(-3, 4, out).astype(f32), a)
        if two and i == len(widths) - 1:
            ly["w2"], ly["b2"] = _sparse_w(rng, two, width), rng.integers(-3, 4, two).astype(f32)
        tower.append(ly)
        width = out
    return tower


def split_input(xfull, Ka):
    """(x0, x1): the columns cut at Ka; Ka = all of them: one block."""
    xfull = np.ascontiguousarray(xfull)
    return (xfull, None) if Ka >= xfull.shape[1] else (np.ascontiguousarray(xfull[:, :Ka]), np.ascontiguousarray(xfull[:, Ka:]))


def exact_input(rng, B, K0):
    return rng.integers(-3, 4, (B, K0)).astype(f32)


def random_input(rng, B, K0):
    return rng.standard_normal((B, K0)).astype(f32)


def _is_int(a):
    a = np.asarray(a, f64)
    return bool(np.all(a == np.rint(a)))


def assert_exact_forward(x, tower):
    """Every operand is an integer and every sum of absolute terms is below 2^24: float32 arithmetic is exact in every order."""
    h = cat_input(x)
    assert _is_int(h)
    for ly in tower:
        assert ly["act"] in ("none", "relu")
        w, b = full_w(ly)
        assert _is_int(w) and _is_int(b)
        assert float((np.abs(h) @ np.abs(w).T + np.abs(b)).max()) < EXACT_LIMIT
        h = act(h @ w.T + b, ly["act"])


def exact_backward_case(rng, B, K0, widths, acts, two=0):
    """(x full [B, K0], tower, hs, dy): integer h with about half of the ReLU units off (they need not be the forward's), integer dy."""
    tower = exact_tower(rng, K0, widths, acts, two)
    hs = []
    for i, (out, a) in enumerate(zip(widths, acts)):
        n = out + (two if i == len(widths) - 1 else 0)
        v = rng.integers(-3, 4, (B, n))
        hs.append((np.maximum(v, 0) if a == "relu" else v).astype(f32))
    dy = rng.integers(-2, 3, (B, widths[-1] + two)).astype(f32)
    return exact_input(rng, B, K0), tower, hs, dy


def random_backward_case(rng, B, K0, widths, acts, two=0):
    tower = random_tower(rng, K0, widths, acts, two)
    hs = []
    for i, (out, a) in enumerate(zip(widths, acts)):
        n = out + (two if i == len(widths) - 1 else 0)
        v = rng.standard_normal((B, n))
        hs.append((np.tanh(v) if a == "tanh" else np.maximum(v, 0) if a == "relu" else v).astype(f32))
    dy = rng.standard_normal((B, widths[-1] + two)).astype(f32)
    return random_input(rng, B, K0), tower, hs, dy


def assert_exact_backward(x, tower, hs, dy):
    xin = cat_input(x)
    B = xin.shape[0]
    dh = np.asarray(dy, f64)
    assert _is_int(xin) and _is_int(dh)
    for l in range(len(tower) - 1, -1, -1):
        ly = tower[l]
        assert ly["act"] in ("none", "relu")
        w, _ = full_w(ly)
        h, hprev = np.asarray(hs[l], f64), (np.asarray(hs[l - 1], f64) if l else xin)
        assert _is_int(h) and _is_int(w)
        g = dh * dact(h, ly["act"])
        assert float((np.abs(g).T @ np.abs(hprev)).max(initial=0)) < EXACT_LIMIT and float(np.abs(g).sum(axis=0).max()) < EXACT_LIMIT
        assert float((np.abs(g) @ np.abs(w)).max()) < EXACT_LIMIT
        dh = g @ w
    return B
