"""The case table of the direct frame-stack tests (tests/stack_cases.py) checked without a GPU: the raw-array reference agrees with
frame_stack_ref.StackRef / obs_layout_ref.expected_layout on what those cover, every case's launch sequence and tactile frames hold what the
table promises (by the record model: without that the GPU comparison could pass while exercising nothing), the coverage check notices a
deleted case, and the table stays small."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import stack_cases as SC  # noqa: E402
from obs_layout_ref import expected_layout  # noqa: E402

TACTILE_CASES = [c for c in SC.CASES if c.tactile]
MAX_CASE_BYTES = 8 << 20            # one run of one case
MAX_TOTAL_BYTES = 64 << 20          # every case, one run each
MAX_LAUNCHES = 3 * 8 + 17           # per case and run: schedule() at n = 8 with a tactile key


def _events(rng, E, steps, H, W, VH, VW, dim):
    """A frame_stack=1 rollout in frame_stack_ref's event format, random frames, with terminal observations for the done envs."""
    def obs():
        return {"tactile": rng.integers(0, 256, (E, H, W, 1), dtype=np.uint8), "visual": rng.integers(0, 256, (E, VH, VW, 3), dtype=np.uint8),
                "oracle": rng.standard_normal((E, dim)).astype(np.float32)}
    ev = [("reset", None, obs())]
    for t in range(steps):
        if t == 3:
            ev.append(("reset", (np.arange(E) % 3 == 1).astype(np.uint8), obs()))
        done = rng.random(E) < 0.3
        o, tm = obs(), obs()
        ev.append(("step", None, o, np.zeros(E, np.float32), done, {int(i): {k: v[i] for k, v in tm.items()} for i in np.nonzero(done)[0]}))
    return ev


@pytest.mark.parametrize("cf", [False, True])
@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_raw_reference_agrees_with_the_rollout_references(n, cf):
    """RawRef fed the same frames as raw arrays (pitch = dim, the visual image of the tactile size or not) gives expected_layout's arrays."""
    rng = np.random.default_rng(n)
    E, dim = 4, 6
    ev = _events(rng, E, 2 * n + 3, 32, 16, 32, 16, dim)
    want = expected_layout(ev, n, cf)
    ref = SC.RawRef(n, cf, {"oracle": dim})
    raw = lambda o: {"tactile": o["tactile"][..., 0], "visual": o["visual"], "oracle": o["oracle"]}   # noqa: E731
    for e, w in zip(ev, want):
        if e[0] == "reset":
            got = ref.reset(raw(e[2]), None if e[1] is None else np.asarray(e[1], bool))
            assert all(np.array_equal(got[k], w[2][k]) and got[k].shape == w[2][k].shape for k in w[2])
        else:
            term = {k: np.stack([e[5][i][k] if i in e[5] else np.zeros_like(e[2][k][0]) for i in range(E)]) for k in e[2]}
            got, gterm = ref.step(raw(e[2]), e[4], raw(term))
            assert all(np.array_equal(got[k], w[2][k]) for k in w[2])
            assert sorted(gterm) == sorted(w[5])
            for i, t in w[5].items():
                assert all(np.array_equal(gterm[i][k], t[k]) and gterm[i][k].shape == t[k].shape for k in t), (i, n, cf)


def test_raw_reference_takes_a_pitch_and_a_visual_size_of_its_own():
    """The two extensions: only the first dim of pitch columns are stacked; the visual image has its own size."""
    rng = np.random.default_rng(0)
    E, n = 3, 3
    ref = SC.RawRef(n, True, {"v0": 3})
    frames = [{"tactile": rng.integers(0, 256, (E, 16, 32), dtype=np.uint8), "visual": rng.integers(0, 256, (E, 5, 48, 3), dtype=np.uint8),
               "v0": rng.integers(0, 1 << 32, (E, 5), dtype=np.uint32)} for _ in range(4)]
    st = ref.reset(frames[0])
    for f in frames[1:]:
        st, _ = ref.step(f, np.zeros(E, bool))
    assert st["tactile"].shape == (E, n, 16, 32) and st["visual"].shape == (E, 3 * n, 5, 48) and st["v0"].shape == (E, 3 * n)
    for s in range(n):
        assert np.array_equal(st["tactile"][:, s], frames[1 + s]["tactile"])
        assert np.array_equal(st["v0"][:, 3 * s:3 * s + 3], frames[1 + s]["v0"][:, :3])
        for c in range(3):
            assert np.array_equal(st["visual"][:, 3 * s + c], frames[1 + s]["visual"][..., c])


def test_record_model_follows_the_stated_rule():
    m = SC.RecModel(3, 2, 1)
    eq = lambda a, b: np.array([[a], [b]], bool)   # noqa: E731
    assert m.update(SC.RESET, np.array([True, True]), eq(1, 0)).tolist() == [[4], [0]]
    assert m.update(SC.STEP, np.array([False, False]), eq(1, 1)).tolist() == [[6], [4]]
    assert m.update(SC.STEP, np.array([False, True]), eq(1, 1)).tolist() == [[7], [4]]        # full; a flagged env starts again from eq
    assert m.update(SC.STEP, np.array([False, False]), eq(0, 1)).tolist() == [[3], [6]]
    assert m.update(SC.RESET, np.array([False, True]), eq(1, 0)).tolist() == [[3], [0]]       # outside the mask: untouched
    assert m.update(SC.STEP, np.array([False, False]), eq(1, 1)).tolist() == [[5], [4]]


def test_names_are_unique_and_shapes_are_what_the_launchers_admit():
    assert len({c.name for c in SC.CASES}) == len(SC.CASES)
    for c in SC.CASES:
        assert c.kind in SC.KINDS and c.keys and 1 <= c.n <= 8 and c.num_envs >= 1, c.name
        if c.tactile:
            H, W = c.tactile
            assert H % 16 == 0 and W % 16 == 0 and (H // 16) * (W // 16) % 16 == 0 and c.n >= 2, c.name
            assert c.num_envs in ((1, 2) if c.tactile == (256, 256) else (1, 3, 5)), c.name
        if c.visual:
            assert c.visual[1] % 16 == 0 and c.kind != "frame" and (c.n >= 2 or c.cf), c.name
        assert all(p >= d >= 0 for d, p in c.vec) and (c.vec == SC.NO_VEC or c.n >= 2), c.name


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_launch_sequence_holds_every_kind_of_launch(case):
    assert SC.schedule_gaps(case) == []
    tmpl, launches = SC.build(case)
    assert len(launches) == SC.launch_count(case) <= MAX_LAUNCHES
    for L in launches:
        for k, (dim, pitch) in zip(("v0", "v1"), case.vec):
            if dim:
                for v in (L.obs[k], L.term[k]):
                    assert (v[:, dim:] == SC.POISON).all() and not (v[:, :dim] == SC.POISON).any()


@pytest.mark.parametrize("case", TACTILE_CASES, ids=lambda c: c.name)
def test_tactile_frames_reach_the_skip_and_its_edges(case):
    tmpl, _ = SC.build(case)
    zero = (SC.blocks_of(tmpl) == 0).all(axis=(-2, -1))
    assert zero.sum() >= 2 and (SC.blocks_of(tmpl)[~zero] != 0).all()
    assert SC.census_gaps(case) == []


def test_census_notices_what_is_missing():
    """The census is not vacuous: with the single-byte steps or the quiet run taken out of a case's frames it reports the gap."""
    case = next(c for c in TACTILE_CASES if c.num_envs >= 3)
    tmpl, launches = SC.build(case)
    saved = [L.obs["tactile"].copy() for L in launches]
    try:
        for L in launches:                                   # no single-byte edit: blocks 12..15 always the template
            for e in range(case.num_envs):
                for b in SC.SINGLE:
                    SC.block_view(L.obs["tactile"][e], b)[:] = SC.block_view(tmpl, b)
        gaps = SC.census_gaps(case)
        assert [g for g in gaps if g[0] == "single"] == [("single", p) for p in range(4)]
        for L in launches:                                   # every block edited in every step: nothing is ever skipped
            L.obs["tactile"][:] ^= 1
        gaps = SC.census_gaps(case)
        assert all(("skip", p) in gaps for p in range(4)) and "refill" in gaps and "zero_reset" in gaps
    finally:
        for L, s in zip(launches, saved):
            L.obs["tactile"][:] = s
    assert SC.census_gaps(case) == []


@pytest.mark.parametrize("case", [c for c in SC.CASES if c.num_envs <= 7 and SC.device_bytes(c) < (1 << 20)][::3], ids=lambda c: c.name)
def test_expected_buffers_keep_what_no_launch_may_touch(case):
    """A self-check of walk() on a sample of the table (every third of the small cases): terminal rows change only for the envs flagged in a step, no stack ever holds the poison, slots zeroed by a done leave after n steps."""
    E, prev = case.num_envs, None
    for L, exp in SC.walk(case):
        flagged = L.flagged(E) if L.mode == SC.STEP else np.zeros(E, bool)
        for k, v in exp.items():
            if k.startswith("v"):
                assert not (v.view(np.uint32) == SC.POISON).any()
            if k.startswith("term_"):
                rows = v.reshape(E, -1)
                if prev is None:
                    assert (rows[~flagged] == SC.FILL).all()
                else:
                    assert np.array_equal(rows[~flagged], prev[k].reshape(E, -1)[~flagged])
        prev = exp


def test_table_covers_every_n_layout_size_and_key_combination():
    assert SC.coverage_gaps(SC.CASES) == []


def test_coverage_check_notices_a_missing_case():
    def without(pred):
        return SC.coverage_gaps([c for c in SC.CASES if not pred(c)])
    for kind in SC.KINDS:
        for n in SC.N_VALUES:
            assert (kind, "n", n) in without(lambda c: c.kind == kind and c.n == n and c.tactile)
            assert (kind, "vector n", n) in without(lambda c: c.kind == kind and c.n == n and c.vec != SC.NO_VEC)
        for hw in SC.TACTILE_SIZES:
            assert (kind, "tactile size", hw) in without(lambda c: c.kind == kind and c.tactile == hw)
        for v in SC.VEC_CONFIGS:
            assert (kind, "vectors", v) in without(lambda c: c.kind == kind and c.vec == v)
        for e in SC.VEC_ENVS:
            assert (kind, "vector envs", e) in without(lambda c: c.kind == kind and c.vec != SC.NO_VEC and c.num_envs == e)
        for keys in ({"tactile"}, {"vec"}) + (({"tactile", "vec"},) if kind == "frame" else ({"visual"}, {"tactile", "visual", "vec"})):
            assert (kind, "keys", tuple(sorted(keys))) in without(lambda c: c.kind == kind and c.keys == keys)
        assert (kind, "one workgroup serving both vector keys") in without(
            lambda c: c.kind == kind and c.vec[0][0] and c.vec[1][0] and (c.num_envs * c.vec[0][0]) % 256)
        if kind == "frame":
            continue
        for n in SC.N_VALUES:
            assert (kind, "visual n", n) in without(lambda c: c.kind == kind and c.n == n and c.visual)
        for hw in SC.VISUAL_SIZES:
            assert (kind, "visual size", hw) in without(lambda c: c.kind == kind and c.visual == hw)
        assert (kind, "a partly filled visual workgroup") in without(lambda c: c.kind == kind and SC.visual_runs(c) % 256)
        assert (kind, "an env boundary inside a wavefront") in without(
            lambda c: c.kind == kind and c.visual and (c.visual[0] * c.visual[1] // 16) % 64 and c.num_envs > 1)
    assert ("obs_cf", "n", 1) in without(lambda c: c.n == 1)


def test_table_stays_small():
    sizes = [SC.device_bytes(c) for c in SC.CASES]
    print(f"{len(SC.CASES)} cases, {sum(SC.launch_count(c) for c in SC.CASES)} launches per run, "
          f"{sum(sizes) / 2 ** 20:.1f} MiB over all cases, largest {max(sizes) / 2 ** 20:.2f} MiB")
    assert max(sizes) <= MAX_CASE_BYTES and sum(sizes) <= MAX_TOTAL_BYTES
    assert all(SC.launch_count(c) <= MAX_LAUNCHES for c in SC.CASES)
