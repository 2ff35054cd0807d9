"""The table of non-finite inputs (tests/nonfinite_cases.py) run without a GPU: the *_device_order restatements stand in the kernels' place
(they are the kernels' bits by tests/test_gpu_sac_loss_abi.py, tests/test_gpu_loss_head_abi.py and tests/test_gpu_nonfinite.py).  Every case
passes check() against the float64 torch composition, torch's float32 composition agrees with the float64 one on every element's class, every
cell of the table is present, and each select the kernels had before (the restatements' mistake=) fails the table at a case named here."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loss_head_ref as ppo_ref  # noqa: E402
import nonfinite_cases as nc  # noqa: E402
import sac_loss_ref as sac_ref  # noqa: E402

torch = pytest.importorskip("torch")

IDS = [e.name for e in nc.ENTRIES]


def _restated(mistake=None):
    return nc.Runner(lambda entry, flat, cfg: entry.restate(flat, cfg, mistake=mistake))


def test_value_class_and_the_three_rules():
    """check() on arrays made by hand: each rule passes what it should and fails on the one element that breaks it."""
    f = lambda *x: np.array(x, np.float32)   # noqa: E731
    d = lambda *x: np.array(x, np.float64)   # noqa: E731
    assert list(nc.value_class([1.0, np.inf, -np.inf, np.nan, 0.0, -0.0])) == [nc.FINITE, nc.POS_INF, nc.NEG_INF, nc.NAN, nc.FINITE, nc.FINITE]
    clean_w, clean_g = dict(x=d(1, 2, 3, 4)), dict(x=f(1, 2, 3, 4))
    want, bound = dict(x=d(1, np.nan, 3.5, np.inf)), dict(x=d(0, 0, 0.25, np.nan))
    t = nc.check(dict(x=f(1, np.nan, 3.75, np.inf)), want, bound, clean_g, clean_w)
    assert t == dict(elements=4, untouched=1, bounded=1, unbounded=0, ratio=1.0)
    for got, rule in ((f(1, 7, 3.5, np.inf), "class"), (f(1, np.nan, 3.5, -np.inf), "class"), (f(1, np.inf, 3.5, np.inf), "class"),
                      (f(1.0000001, np.nan, 3.5, np.inf), "kept its bits"), (f(1, np.nan, 3.8, np.inf), "off by")):
        with pytest.raises(AssertionError, match=rule):
            nc.check(dict(x=got), want, bound, clean_g, clean_w)
    t = nc.check(dict(x=f(1, np.nan, 99, np.inf)), want, dict(x=d(0, 0, np.inf, 0)), clean_g, clean_w)   # a bound that is not finite judges nothing
    assert t["unbounded"] == 1 and t["bounded"] == 0
    with pytest.raises(AssertionError):
        nc.check(dict(x=np.array([1, np.nan, 3.75, np.inf])), want, bound, clean_g, clean_w)               # one dtype for both device runs


@pytest.mark.parametrize("entry", nc.ENTRIES, ids=IDS)
def test_every_cell_is_present_or_carries_its_reason(entry):
    table = nc.cases(entry)
    cells = {c.cell for c in table}
    owed = nc.owed_cells(entry)
    assert owed - cells - set(nc.LEFT_OUT) == set()
    assert cells <= owed                                                      # and no cell that the table does not know
    for cell, reason in nc.LEFT_OUT.items():
        assert cell[2] != "NaN" and cell not in cells and len(reason) > 20, cell
    if hasattr(entry, "table"):
        return
    for name, kind in {x for c in entry.configs for x in entry.inputs(dict(c, B=1))}:   # the full cross of the switches at one position
        for v, _ in nc.VALUES:
            at = [c for c in table if c.input == name and (name, kind) in entry.inputs(c.cfg) and c.value[0] == v and c.cfg["B"] == 257
                  and (kind in ("columns", "scalar") or np.atleast_1d(c.index)[0] == nc.ROWS[nc.CROSS][1])]
            crossed = {tuple(sorted((k, x) for k, x in c.cfg.items() if k != "B")) for c in at}
            owing = [c for c in entry.configs if (name, kind) in entry.inputs(dict(c, B=1))]
            assert len(crossed) == len(owing), (name, v)


def test_the_entries_list_every_array_that_their_generators_draw():
    """inputs() feeds both the table and the cells it owes: held here to the *_inputs generators, which the ABI tests hand to the C entries
    whole."""
    def names(entry, cfg):
        return {n for n, _ in entry.inputs(dict(cfg, B=2))}
    for n in (1, 2, 4):
        want = {f"{k}{i}" if isinstance(v, list) else k for k, v in sac_ref.sac_critic_inputs(2, n, 0).items() for i in range(n if isinstance(v, list) else 1)}
        assert names(nc.SacCritic(n), dict(source="log_ent_coef")) == want | {"log_ent_coef"} and names(nc.SacCritic(n), dict(source="ent_coef")) == want
        want = {f"{k}{i}" if isinstance(v, list) else k for k, v in sac_ref.sac_actor_inputs(2, n, 0).items() for i in range(n if isinstance(v, list) else 1)}
        assert names(nc.SacActor(n), dict(source="log_ent_coef", target_entropy=True)) == want | {"log_ent_coef"}
    want = set(ppo_ref.ppo_inputs(2, 3, True, 0))
    assert names(nc.Ppo(), dict(per_row=True, normalize=True, clip_vf=True)) == want
    assert names(nc.Ppo(), dict(per_row=False, normalize=True, clip_vf=False)) == want - {"old_values"}
    rename = dict(eps="noise_in", g_a="g_actions", g_lp="g_log_prob")
    assert names(nc.Rsample(), dict(clamp=True)) == {rename.get(k, k) for k in ppo_ref.rsample_inputs(2, 3, 0)}
    assert {c.input for c in nc.cases(nc.Gae())} == {"rewards", "values", "episode_starts", "last_values"}        # dones: flag bytes
    assert {c.input for c in nc.cases(nc.VecNorm())} == set(nc.VecNorm().flat(dict(mode="step", done=-1))) - {"dones"}


@pytest.mark.parametrize("entry", nc.ENTRIES, ids=IDS)
def test_the_restatements_pass_every_case_and_torch_float32_agrees_on_the_classes(entry):
    run, table = _restated(), nc.cases(entry)
    for case in table:
        run.run(case)
        flat = case.flat()
        wide, narrow = entry.exact(flat, case.cfg), entry.exact(flat, case.cfg, dtype=torch.float32)
        assert nc.classes_agree({k: wide[k] for k in nc.keys_of(entry, case.cfg)}, narrow) == [], str(case)
    assert run.tally["cases"] == len(table)
    assert run.tally["unbounded"] <= nc.UNBOUNDED.get(entry.name, 0), run.tally
    print(f"{entry.name}: {run.tally}")


def _owners(entry, mistake):
    return [str(c) for c, _ in _restated(mistake).failures(nc.cases(entry))]


def test_fmin_in_the_critics_target_fails_the_table():
    """np.fmin / fminf return the other operand: a NaN in any q_next_c, c = 0 included, left every output finite."""
    assert "fmin drops a NaN" in sac_ref.DEVICE_MISTAKES
    for n in (2, 4):
        owners = _owners(nc.SacCritic(n), "fmin drops a NaN")
        for c in range(n):
            assert f"sac_critic, {n} critics: NaN in q_next{c}[64] (row 64; source=log_ent_coef, B=257)" in owners
        assert all(": NaN in q_next" in o for o in owners) and len(owners) == 8 * n     # every position of every q_next, and nothing else
    assert _owners(nc.SacCritic(1), "fmin drops a NaN") == []                 # one critic: no minimum is taken


def test_the_actors_select_that_skips_a_later_nan_fails_the_table():
    assert "min skips a later NaN" in sac_ref.DEVICE_MISTAKES
    for n in (2, 4):
        owners = _owners(nc.SacActor(n), "min skips a later NaN")
        for c in range(1, n):
            assert f"sac_actor, {n} critics: NaN in q_pi{c}[64] (row 64; source=ent_coef, target_entropy=False, B=257)" in owners
        assert all(": NaN in q_pi" in o and ": NaN in q_pi0" not in o for o in owners) and len(owners) == 9 * (n - 1)


def test_ppos_earlier_selects_fail_the_table():
    """The gate `inside || p1 < p2` gave a row with a NaN ratio or advantage the coefficient 0; the factored d^2 / sigma^2 - 1 kept dlog_std
    finite at sigma = inf and infinite where autograd's two paths give inf - inf."""
    assert ppo_ref.DEVICE_MISTAKES == ("gate drops a NaN", "dlog_std factors the two paths")
    owners = _owners(nc.Ppo(), "gate drops a NaN")
    for o in ("ppo: NaN in old_log_prob[64] (row 64; per_row=True, normalize=True, clip_vf=True, B=257)",
              "ppo: NaN in advantages[64] (row 64; per_row=False, normalize=True, clip_vf=False, B=257)",
              "ppo: +inf in advantages[64] (row 64; per_row=False, normalize=True, clip_vf=False, B=257)",
              "ppo: NaN in mean[64, 0] (row 64, column 0; per_row=True, normalize=False, clip_vf=False, B=257)",
              "ppo: NaN in actions[0, 0] (row 0, column 0; per_row=True, normalize=False, clip_vf=False, B=257)"):
        assert o in owners, o
    owners = _owners(nc.Ppo(), "dlog_std factors the two paths")
    for o in ("ppo: +inf in log_std [B][A][64, 2] (row 64, column A - 1; per_row=True, normalize=False, clip_vf=True, B=257)",
              "ppo: +inf in log_std [A][0] (column 0; per_row=False, normalize=False, clip_vf=False, B=257)",
              "ppo: -inf in old_log_prob[0] (row 0; per_row=True, normalize=False, clip_vf=False, B=257)",
              "ppo: +inf in advantages[64] (row 64; per_row=False, normalize=False, clip_vf=False, B=257)"):
        assert o in owners, o
    assert all("inf in " in o for o in owners)                                # this one needs an infinity; a NaN passes either way


def test_rsamples_backward_that_takes_the_cancelled_paths_as_zero_fails_the_table():
    """The Gaussian sum's gradient, taken analytically, left dmean finite (or infinite) where autograd's G - G is NaN: an infinite noise_in,
    mean or g_log_prob, and log_std = +-inf behind the open clamp."""
    assert ppo_ref.RSAMPLE_DEVICE_MISTAKES == ("cancelled paths taken as 0",)
    owners = _owners(nc.Rsample(), "cancelled paths taken as 0")
    for o in ("rsample: +inf in noise_in[64, 0] (row 64, column 0; clamp=True, B=257)",
              "rsample: -inf in mean[64, 2] (row 64, column A - 1; clamp=False, B=257)",
              "rsample: +inf in log_std[0, 0] (row 0, column 0; clamp=False, B=257)",
              "rsample: -inf in g_log_prob[64] (row 64; clamp=True, B=257)"):
        assert o in owners, o
    assert all("inf in " in o for o in owners) and not any("log_std" in o and "clamp=True" in o for o in owners)


def test_vecnorms_merge_that_steps_from_an_infinite_mean_fails_the_table():
    """One infinity in a chunk that is not the last: the merge's step from an infinite mean is inf - inf, a NaN batch mean where np.mean
    gives the infinity."""
    import vecnorm_ref
    owners = _owners(nc.VecNorm(), vecnorm_ref.DEVICE_MISTAKES[0])
    for o in ("vecnorm: +inf in obs[5, 0] (the first chunk, column 0, step; mode=step, done=-1)",
              "vecnorm: -inf in rewards[300] (a middle chunk, step; mode=step, done=-1)"):
        assert o in owners, o
    assert all("inf in " in o and "the last chunk" not in o and "opposite" not in o for o in owners)
    rng = np.random.default_rng(0)                                            # finite data: the same bits either way
    x = rng.standard_normal((600, 3))
    a, b = vecnorm_ref.device_moments(x), vecnorm_ref.device_moments_before(x)
    assert all(nc._same_bits(p, q).all() for p, q in zip(a, b))


def test_ppos_dlog_std_stays_finite_where_only_the_float32_square_of_sigma_overflows():
    nc.check_ppo_large_log_std(lambda entry, flat, cfg: entry.restate(flat, cfg))


def test_rsamples_float32_underflow_is_pinned_to_torch_float32():
    nc.check_rsample_underflow(lambda entry, flat, cfg: entry.restate(flat, cfg))


def test_the_action_heads_deterministic_product_with_sigma_fails_the_table():
    """x = mean + sigma 0 made a NaN of a finite mean at sigma = inf or NaN, where SB3's mode() is mean itself."""
    assert ppo_ref.head.DEVICE_MISTAKES == ("deterministic multiplies sigma by 0",)
    owners = _owners(nc.ActionHead(), "deterministic multiplies sigma by 0")
    for o in ("action_head: +inf in log_std[64, 0] (row 64, column 0; mode=0, deterministic=True, clamp=False, B=257)",
              "action_head: NaN in log_std[64, 2] (row 64, column A - 1; mode=1, deterministic=True, clamp=False, B=257)"):
        assert o in owners, o
    assert all("in log_std" in o and "deterministic=True" in o for o in owners)


def test_finite_inputs_keep_their_bits_under_the_new_selects():
    """The selects differ from the earlier ones on non-finite values only: on the generators' finite data both give the same bits, a row
    outside the clip whose advantage is exactly 0 (the third branch of the gate) included."""
    for n in (1, 2, 4):
        c, a = nc.SacCritic(n), nc.SacActor(n)
        for entry, mistake, cfg in ((c, "fmin drops a NaN", c.configs[0]), (a, "min skips a later NaN", a.configs[0])):
            flat = entry.flat(dict(cfg, B=257))
            new, old = entry.restate(flat, cfg), entry.restate(flat, cfg, mistake=mistake)
            assert all(nc._same_bits(new[k], old[k]).all() for k in new)
    entry = nc.ActionHead()
    for cfg in entry.configs:
        if cfg["deterministic"]:
            flat = entry.flat(dict(cfg, B=257))
            flat["mean"][0] = [0.0, -0.0, 1.0]
            new, old = entry.restate(flat, dict(cfg, B=257)), entry.restate(flat, dict(cfg, B=257), mistake="deterministic multiplies sigma by 0")
            assert all(nc._same_bits(new[k], old[k]).all() for k in new), cfg
    entry = nc.Rsample()
    for cfg in entry.configs:
        flat = entry.flat(dict(cfg, B=257))
        flat["noise_in"][:2] = [[0.0, -0.0, 0.0], [-0.0, 0.0, -0.0]]          # either zero is saved as it is
        new, old = entry.restate(flat, cfg), entry.restate(flat, cfg, mistake="cancelled paths taken as 0")
        assert all(nc._same_bits(new[k], old[k]).all() for k in new), cfg
        assert nc._same_bits(ppo_ref.rsample_saved_eps(flat["mean"], flat["noise_in"]), flat["noise_in"]).all()
    entry = nc.Ppo()
    for cfg in entry.configs:
        flat = entry.flat(dict(cfg, B=257))
        ratio = entry.exact(flat, cfg)["ratio"]
        below, above = np.flatnonzero(ratio < 1 - nc.CLIP), np.flatnonzero(ratio > 1 + nc.CLIP)
        inside = np.flatnonzero((ratio > 1 - nc.CLIP) & (ratio < 1 + nc.CLIP))
        assert min(len(below), len(above), len(inside)) >= 2
        for rows in (below, above, inside):                                   # an advantage of either zero on each side of the clip and inside
            flat["advantages"][rows[:2]] = [0.0, -0.0]
        new = entry.restate(flat, cfg)
        for mistake in ppo_ref.DEVICE_MISTAKES:
            old = entry.restate(flat, cfg, mistake=mistake)
            assert all(nc._same_bits(new[k], old[k]).all() for k in new), (cfg, mistake)
