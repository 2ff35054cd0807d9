"""The case table of the direct frame-stack tests (tests/test_stack_cases_cpu.py, tests/test_gpu_stack_matrix.py): launch_frame_stack /
k_frame_stack<n> and launch_obs_stack / k_obs_stack<n, cf> (csrc/tg_stack.hip) on raw buffers, through tg_selftest_stack.

A case is a sequence of launches over small buffers.  The reference is frame_stack_ref.StackRef (stable_baselines3's VecFrameStack) and, for
channels first, obs_layout_ref.transpose_image (VecTransposeImage), fed from raw arrays by RawRef: a vector key is the first `dim` of `pitch`
columns, a visual key has a size of its own.  RecModel is the per-block record as the header comment of tg_stack.hip states it, not as the
kernel computes it: bit s = slot s of the block holds the template; after an update the record is `eq` for a flagged env and (rec >> 1) | eq
otherwise, eq = bit n - 1, set iff the new frame's block equals the template's.

Tactile frames are the template with edits, block by block (blocks of 16 x 16 pixels, b = block row * blocks per row + block column; four
blocks share a wavefront, b & 3 is the position inside it):
  blocks 0..3     never edited in the structured envs: once the record is full the kernel skips them, at each of the four positions;
  blocks 5, 10    all zero in the template and never edited: a zeroed slot equals the template there, and must still count as not the template;
  blocks 12..15   equal to the template except for ONE byte, at row 15, column 15 of the block, in one step each, one block at a time (so that
                  each position's 16 bits of the ballot are the only ones set), with the record full; then the template again: the record refills;
  other blocks    random edits in random steps (a whole block or a few bytes).
The last env (with one env: the only env, after the masked reset) gets fully random frames."""
import dataclasses
import functools

import numpy as np

from frame_stack_ref import StackRef
from obs_layout_ref import transpose_image

STEP, RESET = 0, 1                      # StackArgs.mode
FILL = 0x5C                             # what every output buffer holds before the first launch
POISON = np.uint32(0x7FC0DEAD)          # the pitch padding of the vector rows: never in a stack
N_VALUES = tuple(range(2, 9))
TACTILE_SIZES = ((64, 64), (128, 128), (128, 256), (256, 128), (256, 256), (32, 128), (16, 256))
VISUAL_SIZES = ((1, 16), (5, 48), (3, 272), (128, 128))
VEC_CONFIGS = (((40, 40), (0, 0)), ((0, 0), (6, 12)), ((40, 40), (12, 12)), ((3, 5), (3, 12)))    # ((dim0, pitch0), (dim1, pitch1))
NO_VEC = ((0, 0), (0, 0))
VEC_ENVS = (1, 7, 300)
KINDS = ("frame", "obs_cf", "obs_cl")   # launch_frame_stack; launch_obs_stack channels first / last
FLAG_VALUES = (1, 7, 255)
QUIET, ZERO_BLOCKS, SINGLE = (0, 1, 2, 3), (5, 10), (12, 13, 14, 15)
KEYS = ("tactile", "v0", "v1", "visual")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    kind: str
    n: int
    num_envs: int
    tactile: tuple = None               # (H, W) or None
    visual: tuple = None                # (H, W) or None
    vec: tuple = NO_VEC
    seed: int = 0

    @property
    def cf(self):
        return self.kind == "obs_cf"

    @property
    def keys(self):
        return frozenset(k for k, on in (("tactile", self.tactile), ("visual", self.visual), ("vec", self.vec != NO_VEC)) if on)


def _cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, seed=len(out) + 1, **k))   # noqa: E731
    for ki, kind in enumerate(KINDS):
        for i, n in enumerate(N_VALUES):                     # every n with a tactile size of its own; the pairing differs between the kinds
            hw = TACTILE_SIZES[(i + 2 * ki) % 7]
            envs = (1, 2)[(i + ki) % 2] if hw == (256, 256) else (1, 3, 5)[(i + ki) % 3]
            vec = (VEC_CONFIGS + (NO_VEC,))[(i + ki) % 5]
            vis = VISUAL_SIZES[(i + ki) % 4] if kind != "frame" else None
            add(f"{kind}-n{n}-t{hw[0]}x{hw[1]}-e{envs}", kind, n, envs, tactile=hw, visual=vis, vec=vec)
        if kind != "frame":
            add(f"{kind}-n3-tactile-alone", kind, 3, 3, tactile=(128, 256))
            for (hw, envs), n in zip(zip(VISUAL_SIZES, (300, 3, 5, 1)), (2, 5, 7, 4)):   # 45 and 255 runs: part of a workgroup, envs end inside a wavefront
                add(f"{kind}-n{n}-v{hw[0]}x{hw[1]}-e{envs}", kind, n, envs, visual=hw)
        if kind == "obs_cf":
            add("obs_cf-n1-v5x48-e3", kind, 1, 3, visual=(5, 48))
            add("obs_cf-n1-v128x128-e2", kind, 1, 2, visual=(128, 128))
        vec_n = {"frame": (2, 3, 4, 5, 6, 7, 8, 2, 3, 5, 7, 8), "obs_cf": (8, 5, 6, 3), "obs_cl": (4, 7, 5, 8)}[kind]
        pairs = [(v, e) for v in VEC_CONFIGS for e in VEC_ENVS] if kind == "frame" else list(zip(VEC_CONFIGS, (7, 300, 1, 300)))
        for (vec, envs), n in zip(pairs, vec_n):
            add(f"{kind}-n{n}-vec{vec[0][0]}.{vec[0][1]}+{vec[1][0]}.{vec[1][1]}-e{envs}", kind, n, envs, vec=vec)
    return tuple(out)


def schedule(n, num_envs, tactile):
    """[(mode, flag)] of a case: flag None = NULL (every env), else uint8 [num_envs]."""
    E = num_envs
    none = lambda: np.zeros(E, np.uint8)   # noqa: E731

    def some(first):
        f = none()
        idx = np.arange(1, E, 2) if E > 1 else np.arange(1)
        f[idx] = [FLAG_VALUES[(first + k) % 3] for k in range(len(idx))]
        return f

    def every(first):
        return np.array([FLAG_VALUES[(first + k) % 3] for k in range(E)], np.uint8)

    mask = none()
    mask[np.arange(1, E, 3) if E > 1 else np.arange(1)] = 7
    quiet = 2 * n + 5 if tactile else n + 2          # the record fills (n), four single-byte steps, the record refills (n), a skip
    seq = [(RESET, None)] + [(STEP, none()) for _ in range(quiet)]
    seq += [(STEP, some(0)), (STEP, none()), (STEP, every(2)), (STEP, none()), (STEP, none()), (RESET, mask)]
    seq += [(STEP, none()), (STEP, none()), (STEP, None)] + [(STEP, none()) for _ in range(n)] + [(STEP, some(1)), (STEP, none())]
    return seq


def blocks_of(img):
    """[..., H, W] -> [..., nb, 16, 16]"""
    H, W = img.shape[-2:]
    lead = img.shape[:-2]
    return img.reshape(lead + (H // 16, 16, W // 16, 16)).swapaxes(-3, -2).reshape(lead + ((H // 16) * (W // 16), 16, 16))


def block_eq(frames, tmpl):
    """[E][nb] bool: the frame's block equals the template's."""
    return (blocks_of(frames) == blocks_of(tmpl)).all(axis=(-2, -1))


def block_view(img, b):
    """The 16 x 16 view of block b of [H, W] (writable)."""
    bpr = img.shape[1] // 16
    y, x = (b // bpr) * 16, (b % bpr) * 16
    return img[y:y + 16, x:x + 16]


@dataclasses.dataclass
class Launch:
    mode: int
    flag: np.ndarray                    # None: NULL
    obs: dict                           # raw arrays: tactile [E][H][W] u8, v0 / v1 [E][pitch] u32, visual [E][H][W][3] u8
    term: dict                          # the same keys: the terminal frames (steps only; the kernel reads the flagged envs' rows)

    def flagged(self, num_envs):
        return np.ones(num_envs, bool) if self.flag is None else self.flag != 0


@functools.lru_cache(maxsize=2)
def build(case):
    """-> (tmpl or None, [Launch])"""
    rng = np.random.default_rng(1000 + case.seed)
    E, n = case.num_envs, case.n
    seq = schedule(n, E, case.tactile is not None)
    tmpl = None
    if case.tactile:
        H, W = case.tactile
        tmpl = rng.integers(1, 256, (H, W), dtype=np.uint8)
        for b in ZERO_BLOCKS:
            block_view(tmpl, b)[:] = 0
        nb = (H // 16) * (W // 16)
        active = [b for b in range(nb) if b not in QUIET + ZERO_BLOCKS + SINGLE]
    after_mask = False
    launches = []
    for t, (mode, flag) in enumerate(seq):
        after_mask = after_mask or (mode == RESET and flag is not None)
        obs, term = {}, {}
        if case.tactile:
            fr = np.broadcast_to(tmpl, (E, H, W)).copy()
            for e in range(E):
                if (E > 1 and e == E - 1) or (E == 1 and after_mask):
                    fr[e] = rng.integers(0, 256, (H, W), dtype=np.uint8)
                    continue
                for b in active:
                    r = rng.random()
                    if r < 0.25:
                        block_view(fr[e], b)[:] = rng.integers(0, 256, (16, 16), dtype=np.uint8)
                    elif r < 0.5:
                        block_view(fr[e], b)[rng.integers(0, 16, 3), rng.integers(0, 16, 3)] ^= rng.integers(1, 256, 3, dtype=np.uint8)
                for p, b in enumerate(SINGLE):
                    if t == n + 1 + p:
                        block_view(fr[e], b)[15, 15] ^= np.uint8(1 + 37 * p)
            obs["tactile"] = fr
            term["tactile"] = rng.integers(0, 256, (E, H, W), dtype=np.uint8)
        for k, (dim, pitch) in zip(("v0", "v1"), case.vec):
            if dim:
                for d in (obs, term):
                    v = rng.integers(0, 1 << 32, (E, pitch), dtype=np.uint32)
                    v[v == POISON] = 1
                    v[:, dim:] = POISON
                    d[k] = v
        if case.visual:
            obs["visual"] = rng.integers(0, 256, (E,) + case.visual + (3,), dtype=np.uint8)
            term["visual"] = rng.integers(0, 256, (E,) + case.visual + (3,), dtype=np.uint8)
        launches.append(Launch(mode, flag, obs, term))
    return tmpl, launches


class RawRef:
    """StackRef (and, channels first, VecTransposeImage) over raw arrays: every result is the buffer the device holds, as flat bytes per env."""

    def __init__(self, n, channels_first, dims):
        self.ref, self.cf, self.dims = StackRef(n), channels_first, dims      # dims: {"v0": dim, "v1": dim}

    def _obs(self, raw):
        obs = {}
        for k, v in raw.items():
            obs[k] = v[..., None] if k == "tactile" else v[:, :self.dims[k]] if k in self.dims else v
        return obs

    def _frame(self, raw, i):
        return {k: v[i] for k, v in self._obs(raw).items()}

    def _layout(self, k, a):
        return transpose_image(a) if self.cf and k in ("tactile", "visual") else np.ascontiguousarray(a)

    def reset(self, raw, mask=None):
        return {k: self._layout(k, s) for k, s in self.ref.reset(self._obs(raw), mask).items()}

    def step(self, raw, dones, raw_term=None):
        """raw_term None: no terminal stacks.  -> (stacks, {env: {key: terminal stack}})"""
        terminal = {int(i): self._frame(raw_term, i) for i in np.nonzero(dones)[0]} if raw_term is not None else None
        st, term = self.ref.step(self._obs(raw), dones, terminal)
        return ({k: self._layout(k, s) for k, s in st.items()},
                {i: {k: self._layout(k, s) for k, s in t.items()} for i, t in term.items()})


class RecModel:
    def __init__(self, n, num_envs, nb):
        self.n, self.rec = n, np.full((num_envs, nb), FILL, np.uint8)

    def update(self, mode, flagged, eq):
        """flagged [E] bool, eq [E][nb] bool."""
        bit = (eq.astype(np.uint8) << (self.n - 1)).astype(np.uint8)
        f = flagged[:, None]
        if mode == RESET:
            self.rec = np.where(f, bit, self.rec)
        else:
            self.rec = np.where(f, bit, (self.rec >> 1) | bit)
        return self.rec


def walk(case):
    """Yields, per launch: (launch, expected) with expected = {buffer name: bytes as a flat uint8 array} after that launch, for the run WITH
    terminal stacks: "tactile", "v0", "v1", "visual" (stacks), "term_<key>" (terminal stacks: FILL until an env's row is first written, rows of
    unflagged envs as they were), "rec".  The run without terminal stacks expects the same stacks and rec, and never has a terminal stack."""
    tmpl, launches = build(case)
    E = case.num_envs
    ref = RawRef(case.n, case.cf, {k: d for k, (d, _) in zip(("v0", "v1"), case.vec) if d})
    rec = RecModel(case.n, E, tmpl.size // 256) if tmpl is not None else None
    term_bufs = None
    for L in launches:
        flagged = L.flagged(E)
        if L.mode == RESET:
            stacks, terms = ref.reset(L.obs, None if L.flag is None else flagged), {}
        else:
            stacks, terms = ref.step(L.obs, flagged, L.term)
        if term_bufs is None:
            term_bufs = {k: np.full((E, s.nbytes // E), FILL, np.uint8) for k, s in stacks.items()}
        for i, t in terms.items():
            for k, s in t.items():
                term_bufs[k][i] = s.reshape(-1).view(np.uint8)
        exp = {k: s.reshape(-1).view(np.uint8) for k, s in stacks.items()}
        exp.update({"term_" + k: s.reshape(-1).copy() for k, s in term_bufs.items()})
        if rec is not None:
            exp["rec"] = rec.update(L.mode, flagged, block_eq(L.obs["tactile"], tmpl)).reshape(-1).copy()
        yield L, exp


def census(case):
    """What the tactile frames of a case exercise, by the record model: {"skip": positions b & 3 at which an unflagged env's block with a full
    record takes a frame equal to the template; "single": positions of such a block differing in exactly the byte (15, 15); "refill": a block
    that differs once with a full record and is full again exactly n steps later; "zero_reset": an all-zero template block in an env just
    reset; "random_env": an env whose frame differs from the template in every block}."""
    tmpl, launches = build(case)
    E, n = case.num_envs, case.n
    nb, full = tmpl.size // 256, (1 << n) - 1
    rec = RecModel(n, E, nb)
    got = {"skip": set(), "single": set(), "refill": False, "zero_reset": False, "random_env": False}
    zero = (blocks_of(tmpl) == 0).all(axis=(-2, -1))
    pending = {}                                     # (env, block) -> steps since it differed with a full record
    for L in launches:
        flagged, before = L.flagged(E), rec.rec.copy()
        eq = block_eq(L.obs["tactile"], tmpl)
        after = rec.update(L.mode, flagged, eq)
        got["random_env"] |= bool((~eq).all(axis=1).any())
        if L.mode == RESET:
            got["zero_reset"] |= bool((flagged[:, None] & zero[None, :] & eq).any())
            pending.clear()
            continue
        live = ~flagged[:, None] & (before == full)
        for e, b in zip(*np.nonzero(live & eq)):
            got["skip"].add(int(b) & 3)
        diff = blocks_of(L.obs["tactile"]) != blocks_of(tmpl)
        for e, b in zip(*np.nonzero(live & ~eq)):
            if diff[e, b].sum() == 1 and diff[e, b, 15, 15]:
                got["single"].add(int(b) & 3)
        for key in list(pending):
            e, b = key
            if flagged[e] or not eq[e, b]:
                del pending[key]
                continue
            pending[key] += 1
            if pending[key] < n and after[e, b] == full:
                del pending[key]
            elif pending[key] == n:
                got["refill"] |= bool(after[e, b] == full)
                del pending[key]
        for e, b in zip(*np.nonzero(live & ~eq)):
            pending[(int(e), int(b))] = 0
    return got


def census_gaps(case):
    g = census(case)
    return ([("skip", p) for p in range(4) if p not in g["skip"]] + [("single", p) for p in range(4) if p not in g["single"]]
            + [k for k in ("refill", "zero_reset", "random_env") if not g[k]])


def schedule_gaps(case):
    """What the launch sequence of a case lacks."""
    seq = schedule(case.n, case.num_envs, case.tactile is not None)
    E, gaps = case.num_envs, []
    steps = [f for m, f in seq if m == STEP]
    if not (seq[0][0] == RESET and seq[0][1] is None):
        gaps.append("reset of every env with a NULL flag")
    first_run = 0
    for m, f in seq[1:]:
        if m != STEP or f is None or f.any():
            break
        first_run += 1
    if first_run < case.n + 2:
        gaps.append("n + 2 steps")
    if not any(f is not None and not f.any() for f in steps):
        gaps.append("no env flagged")
    if not any(f is not None and f.all() for f in steps) or not any(f is None for f in steps):
        gaps.append("all flagged")
    if E > 1 and not any(f is not None and f.any() and not f.all() for f in steps):
        gaps.append("some flagged")
    masks = [i for i, (m, f) in enumerate(seq) if m == RESET and f is not None and f.any() and (E == 1 or not f.all())]
    if not masks:
        gaps.append("reset with a mask")
    elif not any(m == STEP for m, _ in seq[masks[-1] + 1:]):
        gaps.append("steps after the masked reset")
    seen = {int(v) for _, f in seq if f is not None for v in f}
    if E >= 3 and not {0, 1, 7, 255} <= seen:
        gaps.append("flag values")
    return gaps


def visual_runs(case):
    return case.num_envs * case.visual[0] * case.visual[1] // 16 if case.visual else 0


def coverage_gaps(cases):
    """What a table lacks, as (kind, what) pairs."""
    gaps = []
    for kind in KINDS:
        cs = [c for c in cases if c.kind == kind]
        tact = [c for c in cs if c.tactile]
        vec = [c for c in cs if c.vec != NO_VEC]
        gaps += [(kind, "n", n) for n in N_VALUES if not any(c.n == n for c in tact)]
        gaps += [(kind, "vector n", n) for n in N_VALUES if not any(c.n == n for c in vec)]
        gaps += [(kind, "tactile size", hw) for hw in TACTILE_SIZES if not any(c.tactile == hw for c in tact)]
        gaps += [(kind, "num_envs", e) for e in (1, 3, 5) if not any(c.num_envs == e for c in tact)]
        gaps += [(kind, "vectors", v) for v in VEC_CONFIGS if not any(c.vec == v for c in cs)]
        gaps += [(kind, "vector envs", e) for e in VEC_ENVS if not any(c.num_envs == e for c in vec)]
        if not any(c.vec[0][0] and c.vec[1][0] and (c.num_envs * c.vec[0][0]) % 256 for c in vec):
            gaps.append((kind, "one workgroup serving both vector keys"))
        if not any(p > d for c in vec for d, p in c.vec):
            gaps.append((kind, "pitch > dim"))
        combos = [{"tactile"}, {"vec"}, {"tactile", "vec"}] if kind == "frame" else [{"tactile"}, {"visual"}, {"vec"}, {"tactile", "visual", "vec"}]
        gaps += [(kind, "keys", tuple(sorted(k))) for k in combos if not any(c.keys == k for c in cs)]
        if kind == "frame":
            continue
        vis = [c for c in cs if c.visual]
        gaps += [(kind, "visual n", n) for n in N_VALUES if not any(c.n == n for c in vis)]
        gaps += [(kind, "visual size", hw) for hw in VISUAL_SIZES if not any(c.visual == hw for c in vis)]
        if not any(visual_runs(c) % 256 for c in vis):
            gaps.append((kind, "a partly filled visual workgroup"))
        if not any((c.visual[0] * c.visual[1] // 16) % 64 and c.num_envs > 1 for c in vis):
            gaps.append((kind, "an env boundary inside a wavefront"))
        if kind == "obs_cf" and not any(c.n == 1 for c in vis):
            gaps.append((kind, "n", 1))
    return gaps


def device_bytes(case):
    """Device memory of one run of a case (inputs, stacks, terminal stacks, record), without the guards."""
    E, n, total = case.num_envs, case.n, case.num_envs
    if case.tactile:
        px = case.tactile[0] * case.tactile[1]
        total += px * (2 * E + 1) + 2 * E * px * n + E * px // 256
    for dim, pitch in case.vec:
        total += 4 * E * (2 * pitch + 2 * dim * n)
    if case.visual:
        px = 3 * case.visual[0] * case.visual[1]
        total += 2 * E * px * (1 + n)
    return total


def launch_count(case):
    return len(schedule(case.n, case.num_envs, case.tactile is not None))


CASES = _cases()
