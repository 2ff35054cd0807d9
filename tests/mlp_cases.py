"""The case table of tests/test_gpu_mlp_matrix.py and a plain-Python restatement of the decisions csrc/tg_mlp.hip takes on a case: mlp_plan
(row tiles, G, tiles per workgroup, slabs, workspace), the W staging loop of k_mlp_fwd (`staged`, blocks of 128 rows), the k tiles of k_mlp_bwd
and the waves that own them, the dx skip, and whether and over what k_mlp_reduce runs.  `paths` names the edges a case reaches; EDGES lists
every name, and tests/test_mlp_cases_cpu.py asserts that the table reaches all of them and that no case can be deleted unnoticed.

A case is (B, K0, Ka, [(widths, acts, two), ...]) as in tests/test_gpu_mlp_abi.py: Ka < K0 gives two column blocks, two > 0 a second row block
on the tower's last layer."""
import zlib

import numpy as np

import mlp_ref as ref

R, N = "relu", "none"
ROWS, GROUPS, WAVES, BLOCK = 32, 64, 8, 128          # kMlpRows, kMlpGroups, kMlpWaves, the rows of W staged at a time

# name: (the batch sizes, K0, Ka, towers)
TABLE = {
    "four-mixed": ((33, 65), 40, 33, [([130, 2], [R, N], 0), ([1], [N], 0), ([160, 255, 100], [R, R, N], 100), ([31, 32, 33, 1], [R, N, R, N], 0)]),
    "widest-in": ((33,), 1024, 1024, [([256, 1], [R, N], 0)]),
    "odd-in-three": ((33,), 1023, 1000, [([255, 2], [R, N], 3), ([64], [R], 0), ([1], [N], 0)]),
    "three-tiles": ((4129,), 258, 256, [([256, 256, 1], [R, R, N], 0)]),
    "full-grid": ((2048,), 64, 32, [([33, 2], [R, N], 2)]),
    "grid-plus-one": ((2049,), 64, 33, [([200, 4], [R, N], 0), ([7, 7, 7, 7], [R, R, R, N], 0), ([1], [N], 0), ([96], [R], 32)]),
    "rows-32": ((32,), 64, 1, [([33, 2], [R, N], 0)]),
    "rows-31": ((31,), 64, 63, [([33, 2], [R, N], 0)]),
    "rows-64": ((64,), 2, 1, [([256], [N], 0)]),
    # not in the issue's table: EDGES needs T = 2, and with one row tile k_mlp_reduce runs for the dx row alone
    "two-towers": ((3,), 33, 32, [([31], [R], 1), ([32, 1], [R, N], 0)]),
}
NAMED = [(name, (B, K0, Ka, spec)) for name, (Bs, K0, Ka, spec) in TABLE.items() for B in Bs]
CASES = [case for _, case in NAMED]
HEAVIEST = "three-tiles"
BYTE_CAP = 64 << 20


def case_id(case):
    B, K0, Ka, towers = case
    return f"b{B}-k{K0}" + ("" if Ka == K0 else f"as{Ka}+{K0 - Ka}") + "".join("-" + "x".join(map(str, w)) + (f"+{two}" if two else "") for w, _, two in towers)


def random_acts(acts, t):
    """The random variant rotates the activations, so tanh runs everywhere."""
    return [ref.ACTS[(t + l + 1) % 3] for l in range(len(acts))]


def seed(case, backward=False):
    return zlib.crc32(case_id(case).encode()) + (1 if backward else 0)


def layers_of(case):
    """Per tower a list of (in, out, out2)."""
    _, K0, _, spec = case
    out = []
    for widths, _, two in spec:
        row, width = [], K0
        for i, w in enumerate(widths):
            row.append((width, w, two if i == len(widths) - 1 else 0))
            width = w
        out.append(row)
    return out


def plan(case):
    """mlp_plan: n_tiles, G, the fewest and the most tiles a workgroup walks, slab_floats, ws_floats, dxs_floats."""
    B, K0, _, spec = case
    n_tiles = (B + ROWS - 1) // ROWS
    G = min(n_tiles, GROUPS)
    slab = sum((out + out2) * (k + 1) for tower in layers_of(case) for k, out, out2 in tower)
    T = len(spec)
    return dict(n_tiles=n_tiles, G=G, min_tiles=n_tiles // G, max_tiles=(n_tiles + G - 1) // G, slab_floats=slab,
                ws_floats=G * slab if G > 1 else 0, dxs_floats=T * B * K0 if T > 1 else 0)


def workspace_bytes(case):
    """tg_mlp_backward_workspace."""
    p = plan(case)
    return 4 * (p["ws_floats"] + p["dxs_floats"])


def device_bytes(case):
    """What a backward test of the case holds on the device at once (guard bytes aside): x, the parameters, every h_l, dy, the gradients, dx
    and the workspace."""
    B, K0, _, _ = case
    towers = layers_of(case)
    params = sum((out + out2) * (k + 1) for tower in towers for k, out, out2 in tower)
    hs = B * sum(out + out2 for tower in towers for _, out, out2 in tower)
    dys = B * sum(tower[-1][1] + tower[-1][2] for tower in towers)
    return 4 * (B * K0 + 2 * params + hs + dys + B * K0) + workspace_bytes(case)


def tiles_of_group(case, grp):
    """The row tiles workgroup grp walks, ascending."""
    p = plan(case)
    return list(range(grp, p["n_tiles"], p["G"]))


def straddling_tile(K0, Ka):
    """The k tile of layer 0 that holds columns of both blocks, or None."""
    kt = Ka // ROWS
    return kt if Ka < K0 and Ka % ROWS else None


def skipped_dx_tiles(case, want_dx):
    """The k tiles of layer 0 the dx skip of k_mlp_bwd passes over (T = 1 only)."""
    _, K0, Ka, spec = case
    if len(spec) != 1:
        return []
    want0, want1 = want_dx[0], want_dx[1] and Ka < K0
    return [kt for kt in range((K0 + 31) // 32) if (not want0 and kt * 32 + 32 <= Ka) or (not want1 and kt * 32 >= Ka)]


EDGES = (
    "T=1", "T=2", "T=3", "T=4", "depth=1", "depth=2", "depth=3", "depth=4", "mixed depths",
    "G=1", "1<G=n_tiles<64", "G=64, one tile each", "G=64, 1 or 2 tiles each", "G=64, 2 or 3 tiles each", "a workgroup walks three tiles",
    "last tile full, G=1", "last tile full, 1<G<64", "last tile full, G=64", "last tile has 31 rows", "last tile has 1 row",
    "in odd", "in%32=0", "in%32=1", "in%32=31", "K0=1024", "K0=1023", "fwd: 32 staging chunks", "bwd: four k tiles a wave",
    "outT%32=0", "outT%32=1", "outT%32=31", "128<outT<256, outT%32!=0", "outT=255", "outT=31", "outT=32",
    "staging: one block", "staging: partial second block", "staging: two full blocks",
    "second block starts at a multiple of 32", "second block starts inside a 32-column group", "second block crosses column 128",
    "partial reload, more than two dweight tiles", "partial reload, K0>32",
    "T=1: dx written by k_mlp_bwd", "T>1: dx from the towers' slabs", "T>1: a block not asked for", "no dx: layer 0 stops before dh_0",
    "dx tile skipped", "straddling tile, both blocks", "straddling tile, dx0 only", "straddling tile, dx1 only",
    "blocks meet at a tile edge, one block only", "Ka=1",
    "no reduce", "reduce with the dx row", "reduce without the dx row", "reduce: the dx row alone (G=1)",
    "reduce: more than 12 segments",
    "frozen layer, G>1", "dweight2 without dweight, G>1", "bias only, G>1", "NULL dy, G>1",
)


def paths(case, want_dx=(True, True), skip=(), null_dy=()):
    """The set of EDGES the case reaches in tg_mlp_forward and tg_mlp_backward.  skip: {(t, l): the gradient names still given} (a plain set
    of (t, l): none given); null_dy: the towers whose dy is NULL."""
    B, K0, Ka, spec = case
    skip = dict(skip) if isinstance(skip, dict) else {key: () for key in skip}
    p, towers, T = plan(case), layers_of(case), len(spec)
    G, n_tiles = p["G"], p["n_tiles"]
    want0, want1 = bool(want_dx[0]), bool(want_dx[1]) and Ka < K0
    got = {f"T={T}"} | {f"depth={len(tower)}" for tower in towers}
    if len({len(tower) for tower in towers}) > 1:
        got.add("mixed depths")
    # mlp_plan
    if G == 1:
        got.add("G=1")
    elif n_tiles < GROUPS:
        got.add("1<G=n_tiles<64")
    else:
        got.add({(1, 1): "G=64, one tile each", (1, 2): "G=64, 1 or 2 tiles each", (2, 3): "G=64, 2 or 3 tiles each"}[(p["min_tiles"], p["max_tiles"])])
    if p["max_tiles"] >= 3:
        got.add("a workgroup walks three tiles")
    last_rows = B - (n_tiles - 1) * ROWS
    if last_rows == ROWS:
        got.add("last tile full, G=1" if G == 1 else "last tile full, 1<G<64" if n_tiles < GROUPS else "last tile full, G=64")
    elif last_rows in (1, 31):
        got.add(f"last tile has {last_rows} row" + ("s" if last_rows > 1 else ""))
    # per layer: the k loop and the W staging loop of k_mlp_fwd, the tiles of k_mlp_bwd
    for t, tower in enumerate(towers):
        for l, (k, out, out2) in enumerate(tower):
            outT, nkt = out + out2, (k + 31) // 32
            staged = (outT + 31) // 32 * 32
            if k % 2:
                got.add("in odd")
            if k % 32 in (0, 1, 31):
                got.add(f"in%32={k % 32}")
            if l == 0 and k in (1023, 1024):
                got.add(f"K0={k}")
            if nkt == 32:
                got.update(("fwd: 32 staging chunks", "bwd: four k tiles a wave"))         # kt = wave, wave + 8, wave + 16, wave + 24
            if outT % 32 in (0, 1, 31):
                got.add(f"outT%32={outT % 32}")
            if 128 < outT < 256 and outT % 32:
                got.add("128<outT<256, outT%32!=0")
            if outT in (255, 31, 32):
                got.add(f"outT={outT}")
            got.add("staging: one block" if staged <= BLOCK else "staging: two full blocks" if staged == 2 * BLOCK else "staging: partial second block")
            if out2:
                got.add("second block starts inside a 32-column group" if out % 32 else "second block starts at a multiple of 32")
                if out < 128 < outT:
                    got.add("second block crosses column 128")
            kept = skip.get((t, l))
            wants_w = kept is None or "dweight" in kept or "dweight2" in kept
            if p["max_tiles"] >= 2 and wants_w:                                            # acc[i] = sw[co * in + k] runs
                if ((outT + 31) // 32) * nkt > 2:
                    got.add("partial reload, more than two dweight tiles")
                if l == 0 and k > 32:
                    got.add("partial reload, K0>32")
            if kept is not None and G > 1:
                if not kept:
                    got.add("frozen layer, G>1")
                elif "dweight2" in kept and "dweight" not in kept and out2:
                    got.add("dweight2 without dweight, G>1")
                elif not wants_w:
                    got.add("bias only, G>1")
        if t in null_dy and G > 1:
            got.add("NULL dy, G>1")
    # dx
    straddle = straddling_tile(K0, Ka)
    if not (want0 or want1):
        got.add("no dx: layer 0 stops before dh_0")
    else:
        got.add("T=1: dx written by k_mlp_bwd" if T == 1 else "T>1: dx from the towers' slabs")
        if T > 1 and Ka < K0 and want0 != want1:
            got.add("T>1: a block not asked for")
        if T == 1 and skipped_dx_tiles(case, (want0, want1)):
            got.add("dx tile skipped")
        if straddle is not None:
            got.add("straddling tile, both blocks" if want0 and want1 else "straddling tile, dx0 only" if want0 else "straddling tile, dx1 only")
        if Ka < K0 and Ka % 32 == 0 and want0 != want1:
            got.add("blocks meet at a tile edge, one block only")
    if Ka == 1:
        got.add("Ka=1")
    # k_mlp_reduce
    sum_dx = T > 1 and (want0 or want1)
    if G == 1 and not sum_dx:
        got.add("no reduce")
    else:
        got.add("reduce: the dx row alone (G=1)" if G == 1 else "reduce with the dx row" if sum_dx else "reduce without the dx row")
        if G > 1 and 2 * sum(len(tower) for tower in towers) > 12:
            got.add("reduce: more than 12 segments")
    assert got <= set(EDGES), got - set(EDGES)
    return got


# ------------------------------------------------------------------------------------------------------------------ the option runs
STRADDLES = ((33, 7), (1, 39), (32, 8))              # (Ka, Kb) of the dx runs: a straddling tile, Ka = 1, the blocks meeting at a tile edge
PARTIAL_DX = ((True, False), (False, True), (False, False))
FROZEN = {(0, 0): (), (3, 0): ("dweight2", "dbias2"), (1, 2): ("dbias",)}     # on grid-plus-one: what each layer is still given
FROZEN_NULL_DY = (2,)


def dx_runs():
    """(case, want_dx) of the dx-block runs: tower 0 of four-mixed alone (k_mlp_bwd writes dx and skips tiles), then all four (the dxs path)."""
    _, K0, _, spec = TABLE["four-mixed"]
    return [((65, K0, Ka, towers), want) for Ka, Kb in STRADDLES for towers in (spec[:1], spec) for want in PARTIAL_DX]


def option_runs():
    """(the table's case it stands on, case, paths' keyword arguments) of every option run of tests/test_gpu_mlp_matrix.py."""
    runs = [("four-mixed", case, dict(want_dx=want)) for case, want in dx_runs()]
    Bs, K0, Ka, spec = TABLE["grid-plus-one"]
    runs.append(("grid-plus-one", (Bs[0], K0, Ka, spec), dict(skip=FROZEN, null_dy=FROZEN_NULL_DY)))
    return runs


def reached(without=None):
    """The union of paths over the table and the option runs, without one of the table's names."""
    got = set()
    for name, case in NAMED:
        if name != without:
            got |= paths(case)
    for name, case, kw in option_runs():
        if name != without:
            got |= paths(case, **kw)
    return got


# ------------------------------------------------------------------------------------------------------------------ the draws
def forward_variants(case):
    """((x, towers) exact, (x, towers) random) from the seed of the case: what the GPU test runs and the CPU test checks for exactness."""
    B, K0, Ka, spec = case
    rng = np.random.default_rng(seed(case))
    exact = (ref.split_input(ref.exact_input(rng, B, K0), Ka), [ref.exact_tower(rng, K0, w, a, two) for w, a, two in spec])
    rand = (ref.split_input(ref.random_input(rng, B, K0), Ka), [ref.random_tower(rng, K0, w, random_acts(a, t), two) for t, (w, a, two) in enumerate(spec)])
    return exact, rand


def backward_variants(case):
    """((x, towers, hs, dys) exact, the same random): the towers share the first tower's input draw, as in tests/test_gpu_mlp_abi.py."""
    B, K0, Ka, spec = case
    rng = np.random.default_rng(seed(case, backward=True))
    out = []
    for exact in (True, False):
        xs, towers, hs, dys = None, [], [], []
        for t, (w, a, two) in enumerate(spec):
            if exact:
                xfull, tower, h, dy = ref.exact_backward_case(rng, B, K0, w, a, two)
            else:
                xfull, tower, h, dy = ref.random_backward_case(rng, B, K0, w, random_acts(a, t), two)
            xs = xfull if xs is None else xs
            towers.append(tower), hs.append(h), dys.append(dy)
        out.append((ref.split_input(xs, Ka), towers, hs, dys))
    return tuple(out)
