"""The case tables of the direct exchange tests (tests/exchange_cases.py) checked without a GPU: tests/exchange_ref.py agrees with the
package's torch definition of the tile message (parallel.torch_pack_tiles / torch_unpack_tiles) on what that covers, every case round-trips,
the two forms of the multi-rank unpack agree after every message, every wrong variant of exchange_ref is told from the right answer by a named
case (without that the GPU comparison could pass while separating nothing), the coverage check notices a deleted case, and the tables stay
small."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import exchange_cases as XC  # noqa: E402
import exchange_ref as ref  # noqa: E402

MAX_TOTAL_BYTES = 128 << 20         # every case of CASES, SEQUENCES and MALFORMED, one run each
MAX_LARGE_BYTES = 320 << 20         # the one large case
MAX_COPY_BYTES = 2 * ((16 << 20) + 21 + 4097)    # the largest copy: source and destination

# variant -> a case that must separate it (names of CASES, SEQUENCES or MALFORMED)
SEPARATED_BY = {
    "tiles_per_row_from_h": "t2-16x32-n2-all",
    "last_group_dropped": "t65-80x208-n5-one_last",
    "liveness_first_word_only": "t1-16x16-n257-single_byte",
    "tail_whole_words_only": None,              # filled below: every case whose tail has a sub-16 rest
    "no_restore": "r2-skip-1-80x208-n3",
    "skip_rank_written": "r3-skip1-16x16-n5",
    "count_unclamped_ids_signed": "16x16-n5-ids",
}


def _run_sequence(seq, with_list, wrong=None, dst_fill=None):
    """The destinations after each message, and the model."""
    tmpl, images, messages = XC.build_sequence(seq)
    dst = np.broadcast_to(tmpl, (seq.n_ranks, seq.n_images, seq.h, seq.w)).copy()
    if not with_list or dst_fill is not None:
        dst[:] = XC.FILL if dst_fill is None else dst_fill
    if 0 <= seq.skip_rank < seq.n_ranks:
        dst[seq.skip_rank] = XC.SKIP_FILL
    lists = np.zeros((seq.n_ranks, 1 + seq.n_images * seq.T), np.uint32)
    if 0 <= seq.skip_rank < seq.n_ranks:
        lists[seq.skip_rank] = 0xA5A5A5A5
    um = ref.UnpackMulti(tmpl, seq.n_ranks, seq.n_images, seq.h, seq.w, seq.skip_rank, with_list, dst, lists if with_list else None, wrong)
    return [um.step(messages[m]).copy() for m in range(XC.N_MESSAGES)], um


@pytest.mark.parametrize("case", [c for c in XC.CASES if c.T <= 81], ids=lambda c: c.name)
def test_reference_agrees_with_the_torch_definition(case):
    torch = pytest.importorskip("torch")
    from tactile_gym_amd.parallel import torch_pack_tiles, torch_unpack_tiles
    tmpl, img = XC.build(case)[:2]
    hdr, rec = ref.pack(img, tmpl)
    cap = ref.capacity(case.n_images, case.h, case.w)
    dst = torch.zeros(cap, dtype=torch.uint8)
    count = torch_pack_tiles(torch, torch.from_numpy(img), torch.from_numpy(tmpl).reshape(-1), dst)
    assert count == hdr[0] == len(rec)
    assert np.array_equal(dst.numpy()[:16 + rec.size], ref.message(hdr, rec))
    out = torch.zeros((case.n_images, case.h * case.w), dtype=torch.uint8)
    torch_unpack_tiles(torch, torch.from_numpy(ref.message(hdr, rec)), torch.from_numpy(tmpl).reshape(-1), case.n_images, case.h, case.w, out)
    assert np.array_equal(out.numpy().reshape(img.shape), img)


def test_the_torch_definition_handles_a_non_square_image():
    torch = pytest.importorskip("torch")
    from tactile_gym_amd.parallel import torch_pack_tiles
    rng = np.random.default_rng(0)
    tmpl = XC.template_of(48, 80, 1)
    img = XC._mixed(rng, tmpl, 3)
    hdr, rec = ref.pack(img, tmpl)
    dst = torch.zeros(ref.capacity(3, 48, 80), dtype=torch.uint8)
    assert torch_pack_tiles(torch, torch.from_numpy(img), torch.from_numpy(tmpl).reshape(-1), dst) == len(rec)
    assert np.array_equal(dst.numpy()[:16 + rec.size], ref.message(hdr, rec))


@pytest.mark.parametrize("case", XC.CASES, ids=lambda c: c.name)
def test_round_trip_and_the_promised_content(case):
    tmpl, img, tail, off, nbytes = XC.build(case)
    assert tmpl.any() and not tmpl.all()
    hdr, rec = ref.pack(img, tmpl)
    assert hdr.tolist() == [len(rec), case.n_images, case.T, ref.MAGIC] and not rec[:, 4:16].any()
    ids = rec[:, :4].copy().view(np.uint32).reshape(-1)
    assert (np.diff(ids.astype(np.int64)) > 0).all() and len(rec) == XC.live_count(tmpl, img)
    msg = XC.expected_message(case)
    assert np.array_equal(ref.unpack(msg, tmpl, case.n_images, case.h, case.w), img)
    assert np.array_equal(ref.unpack(msg[:16 + rec.size], tmpl, case.n_images, case.h, case.w), img)
    want = {"none": [], "all": list(range(case.n_images * case.T)), "one_first": [0], "one_last": [case.n_images * case.T - 1],
            "one_lane63": [(case.n_images - 1) * case.T + 63], "single_byte": list(range(case.n_images * case.T))}
    if case.content in want:
        assert ids.tolist() == want[case.content]
    else:
        assert 0 < len(ids) < case.n_images * case.T or case.n_images * case.T <= 2
    if case.content == "all":
        assert 16 + rec.size == ref.capacity(case.n_images, case.h, case.w)          # the message ends exactly at the capacity
    assert off % 16 == 0 and off >= ref.capacity(case.n_images, case.h, case.w) and nbytes > off + (len(tail) if tail is not None else 0)
    assert (msg[16 + rec.size:off] == XC.FILL).all() and (msg[off + (len(tail) if tail is not None else 0):] == XC.FILL).all()


def test_mixed_cases_hold_template_tiles_next_to_zero_tiles():
    for case in XC.CASES:
        if case.content != "mixed" or case.n_images * case.T < 16:
            continue
        tmpl, img = XC.build(case)[:2]
        tv, tt = XC._tiles_view(img), XC._tiles_view(np.broadcast_to(tmpl, img.shape))
        is_tmpl, is_zero = (tv == tt).all(axis=(3, 4)), (tv == 0).all(axis=(3, 4))
        assert (is_tmpl & ~is_zero).any() and (is_zero & ~is_tmpl).any() and (is_zero & is_tmpl).any() == bool((tt == 0).all(axis=(3, 4)).any()), case.name


@pytest.mark.parametrize("seq", XC.SEQUENCES, ids=lambda s: s.name)
def test_both_forms_of_the_multi_unpack_agree_after_every_message(seq):
    tmpl, images, messages = XC.build_sequence(seq)
    fill, _ = _run_sequence(seq, False)
    keep, um = _run_sequence(seq, True)
    live_seen = np.zeros((seq.n_ranks, seq.n_images * seq.T), int)
    for m in range(XC.N_MESSAGES):
        assert np.array_equal(fill[m], keep[m]), m
        for r in range(seq.n_ranks):
            if r == seq.skip_rank:
                assert (fill[m][r] == XC.SKIP_FILL).all()
                continue
            assert np.array_equal(fill[m][r], images[m][r]), (m, r)
            assert messages[m][r].size == seq.stride > ref.capacity(seq.n_images, seq.h, seq.w)
    for r in range(seq.n_ranks):
        kinds = seq.kinds(r)
        if kinds is None:
            assert (um.lists[r] == 0xA5A5A5A5).all()
            continue
        for m, kind in enumerate(kinds):
            live_seen[r] = live_seen[r] * 2 + (XC._tiles_view(images[m][r]) != XC._tiles_view(np.broadcast_to(tmpl, images[m][r].shape))
                                               ).any(axis=(3, 4)).reshape(-1)
        # a tile live, then not, then live again: bits ..101.. in some tile's history
        hist = live_seen[r]
        assert any(((hist >> s) & 7 == 5).any() for s in range(3)) or seq.n_images * seq.T < 3, (seq.name, r)
    # the list form touches nothing but the previous and the new tiles: a destination that never held the template keeps its bytes elsewhere
    stale, _ = _run_sequence(seq, True, dst_fill=0x3C)
    for r in range(seq.n_ranks):
        if r == seq.skip_rank:
            continue
        ever = (live_seen[r] != 0).reshape(seq.n_images, seq.h // 16, seq.w // 16)
        tv = XC._tiles_view(stale[-1][r])
        assert (tv[~ever] == 0x3C).all() and np.array_equal(tv[ever], XC._tiles_view(images[-1][r])[ever])


def test_bad_headers_leave_the_template_and_an_empty_list():
    seq = next(s for s in XC.SEQUENCES if s.n_ranks == 3 and s.skip_rank == -1)
    tmpl, images, messages = XC.build_sequence(seq)
    um = ref.UnpackMulti(tmpl, 3, seq.n_images, seq.h, seq.w, -1, True)
    for m in range(XC.N_MESSAGES):
        um.step(messages[m])
        for r in range(3):
            kind = seq.kinds(r)[m]
            if kind in ("bad_magic", "wrong_t"):
                assert um.lists[r][0] == 0 and (um.dst[r] == tmpl).all()
            elif kind == "all_ff":
                assert um.lists[r][0] == seq.n_images * seq.T and messages[m][r][:4].view(np.uint32)[0] == 0xFFFFFFFF


@pytest.mark.parametrize("mal", XC.MALFORMED, ids=lambda m: m.name)
def test_malformed_messages_are_what_they_claim(mal):
    tmpl, want, msg = XC.build_malformed(mal)
    got = ref.unpack(msg, tmpl, mal.n_images, mal.h, mal.w)
    assert np.array_equal(got, want)
    hdr = msg[:16].view(np.uint32)
    room = (len(msg) - 16) // ref.REC
    assert min(int(hdr[0]), mal.n_images * mal.T) <= room
    if mal.what == "ids":
        ok, ids, _ = ref.read_records(msg, mal.n_images, mal.T)
        assert ok and set(mal.bad_ids) <= set(ids.tolist()) and len(ids) == hdr[0] <= mal.n_images * mal.T
        pos = [int(np.nonzero(ids == b)[0][0]) for b in mal.bad_ids]
        assert 0 < min(pos) and max(pos) < len(ids) - 1                  # among valid records
        assert not (want == tmpl).all()
        if mal.T == 1:      # under a signed check the store stays inside the leading guard of the destination's allocation
            assert all(0 < (2 ** 32 - b) * 256 <= 4096 - 256 for b in mal.bad_ids)
        else:               # and at T >= 2 no id is negative after the division
            assert all(b // mal.T < 2 ** 31 for b in mal.bad_ids)


def _separating(variant):
    """Names of the table entries on which the wrong variant gives another answer than the right one."""
    out = []
    if variant in ("tiles_per_row_from_h", "last_group_dropped", "liveness_first_word_only", "tail_whole_words_only"):
        for c in XC.CASES:
            if not np.array_equal(XC.expected_message(c), XC.expected_message(c, wrong=variant)):
                out.append(c.name)
    if variant in ("no_restore", "skip_rank_written"):
        for s in XC.SEQUENCES:
            right, um = _run_sequence(s, True)
            wrong, wm = _run_sequence(s, True, wrong=variant)
            if any(not np.array_equal(a, b) for a, b in zip(right, wrong)) or not np.array_equal(um.lists, wm.lists):
                out.append(s.name)
    if variant in ("count_unclamped_ids_signed", "tiles_per_row_from_h"):
        for m in XC.MALFORMED:
            tmpl, want, msg = XC.build_malformed(m)
            if not np.array_equal(ref.unpack(msg, tmpl, m.n_images, m.h, m.w, wrong=variant), want):
                out.append(m.name)
    return out


@pytest.mark.parametrize("variant", ref.WRONG)
def test_every_wrong_variant_is_separated(variant):
    names = _separating(variant)
    print(f"{variant}: separated by {len(names)} entries: {names[:12]}")
    assert names, variant
    if variant == "tail_whole_words_only":
        want = [c.name for c in XC.CASES if max(XC.tail_of(c)[0], 0) % 16]
        assert want and names == want
    else:
        assert SEPARATED_BY[variant] in names
    if variant == "tiles_per_row_from_h":        # every non-square shape of the table, and no square one
        assert {n for n in names if n.startswith("t")} >= {c.name for c in XC.CASES if c.h != c.w and c.content == "all"}
        assert not any(c.name in names for c in XC.CASES if c.h == c.w)
    if variant == "last_group_dropped":
        assert all(c.name in names for c in XC.CASES if c.content in ("all", "one_last") and c.T % 64)      # a partly filled last group
        assert not any(c.name in names for c in XC.CASES if c.T % 64 == 0)
    if variant == "liveness_first_word_only":
        assert all(c.name in names for c in XC.CASES if c.content == "single_byte")
    if variant == "no_restore":
        assert all(s.name in names for s in XC.SEQUENCES if s.skip_rank != 0 or s.n_ranks > 1)
    if variant == "skip_rank_written":
        assert names == [s.name for s in XC.SEQUENCES if s.skip_rank >= 0]
    if variant == "count_unclamped_ids_signed":
        assert names == [m.name for m in XC.MALFORMED if m.what == "ids" and m.T == 1]


def test_names_are_unique_and_shapes_are_what_the_entries_admit():
    names = [c.name for c in XC.CASES + XC.SEQUENCES + XC.MALFORMED]
    assert len(set(names)) == len(names)
    for c in XC.CASES + XC.SEQUENCES + XC.MALFORMED:
        assert c.h % 16 == 0 and c.w % 16 == 0 and c.h > 0 and c.w > 0 and c.n_images >= 1, c.name
    for s in XC.SEQUENCES:
        assert -1 <= s.skip_rank < s.n_ranks and s.stride % 16 == 0, s.name


def test_the_large_case_crosses_every_block_cap():
    tmpl, img = XC.build_large()
    live = XC.live_count(tmpl, img)
    print(f"large case: {XC.LARGE.n_images} images, {img.nbytes / 2 ** 20:.1f} MiB, {live} live tiles of {XC.LARGE.n_images * XC.LARGE.T}")
    assert img.nbytes > 32 << 20 and 65536 < live < XC.LARGE.n_images * XC.LARGE.T
    assert sorted(XC.caps_crossed(XC.LARGE, live)) == sorted(k for k in XC.BLOCK_CAPS if k != "k_copy_bytes")
    for c in XC.CASES:                                    # and no other case crosses any
        assert XC.caps_crossed(c, c.n_images * c.T) == [], c.name
    cap = XC.BLOCK_CAPS["k_copy_bytes"][0] * XC.BLOCK_CAPS["k_copy_bytes"][1]
    assert max(XC.COPY_SIZES) > cap


def test_block_caps_are_those_of_the_source():
    """BLOCK_CAPS restates numbers of tg_exchange.hip's launch code: each cap appears there as `< cap ? ... : cap`."""
    src = open(os.path.join(HERE, "..", "tactile_gym_amd", "csrc", "tg_exchange.hip")).read()
    for cap in {v[0] for v in XC.BLOCK_CAPS.values()}:
        assert f"< {cap} ?" in src and f": {cap})" in src, cap
    assert src.count("< 4096 ?") == 3 and src.count("< 1024 ?") == 1 and src.count("< 2048 ?") == 1 and src.count("< 8192 ?") == 1


def test_tables_cover_every_edge():
    assert XC.coverage_gaps(XC.CASES) == []


def test_coverage_check_notices_a_missing_case():
    def without(pred):
        return XC.coverage_gaps([c for c in XC.CASES if not pred(c)])
    for T, hw in XC.SHAPES.items():
        assert ("T", T) in without(lambda c: (c.h, c.w) == hw)
        for n in ((1, 3) if T == 256 else (1, 2)):
            assert ("n_images", T, n) in without(lambda c: (c.h, c.w) == hw and c.n_images == n)
        if T <= 81:
            assert ("n_images", T, "odd >= 5") in without(lambda c: (c.h, c.w) == hw and c.n_images >= 5)
        for content in XC.CONTENTS:
            if content != "one_lane63" or T >= 64:
                assert ("content", T, content) in without(lambda c: (c.h, c.w) == hw and c.content == content)
    assert ("H > W",) in without(lambda c: c.h > c.w)
    assert ("W > H",) in without(lambda c: c.w > c.h)
    assert ("non-square shapes", 2) in without(lambda c: c.h != c.w and (c.h, c.w) not in ((16, 32), (64, 16)))
    for s in XC.TAIL_SIZES + (XC.NULL_TAIL,):
        assert ("tail", s) in without(lambda c: XC.tail_of(c)[0] == s)
    assert ("tail offsets",) in without(lambda c: XC.tail_of(c)[1] == 32)
    for n_ranks in (1, 2, 3):
        for skip in {-1, 0, n_ranks // 2, n_ranks - 1}:
            seqs = [s for s in XC.SEQUENCES if not (s.n_ranks == n_ranks and s.skip_rank == skip)]
            assert ("sequence", n_ranks, skip) in XC.coverage_gaps(XC.CASES, sequences=seqs)
    assert ("sequence", "T = 1") in XC.coverage_gaps(XC.CASES, sequences=[s for s in XC.SEQUENCES if s.T != 1])
    one_rank = [s for s in XC.SEQUENCES if s.n_ranks - (s.skip_rank >= 0) <= 1]
    assert ("sequence kind", "wrong_t") in XC.coverage_gaps(XC.CASES, sequences=one_rank)
    mal = [m for m in XC.MALFORMED if not (m.what == "ids" and m.T == 1)]
    assert ("malformed id", 1, 0xFFFFFFF1) in XC.coverage_gaps(XC.CASES, malformed=mal)
    assert ("malformed id", "T >= 2") in XC.coverage_gaps(XC.CASES, malformed=[m for m in XC.MALFORMED if m.T == 1])
    for w in ("bad_magic", "wrong_t", "count_ff", "count_cap_plus_1"):
        assert ("malformed header", w) in XC.coverage_gaps(XC.CASES, malformed=[m for m in XC.MALFORMED if m.what != w])
    for s in XC.COPY_SIZES:
        assert ("copy size", s) in XC.coverage_gaps(XC.CASES, copy_sizes=[x for x in XC.COPY_SIZES if x != s])
    cap = 16 << 20
    pairs = lambda pred: XC.coverage_gaps(XC.CASES, copy_pairs=[p for p in XC.COPY_PAIRS if not pred(*p)])   # noqa: E731
    assert ("copy pair", "an empty member") in pairs(lambda a, b: a == 0 and b > 0)
    assert ("copy pair", "two tails") in pairs(lambda a, b: a % 16 and b % 16)
    assert ("copy pair", "the sum crosses the cap") in pairs(lambda a, b: a < cap and b < cap and a + b > cap)


def test_single_byte_census_notices_a_missing_position():
    case = next(c for c in XC.CASES if c.content == "single_byte" and c.T == 9)
    assert XC.single_byte_census(case) == (set(range(256)), {1, 128})
    short = XC.Case("short", case.h, case.w, 5, "single_byte", seed=case.seed)
    pos, _ = XC.single_byte_census(short)
    assert len(pos) == 45
    assert XC.single_byte_census(next(c for c in XC.CASES if c.content == "mixed" and c.T == 9)) is None


def test_table_stays_small():
    entries = XC.CASES + XC.SEQUENCES + XC.MALFORMED
    sizes = [XC.device_bytes(c) for c in entries]
    large = XC.device_bytes(XC.LARGE)
    print(f"{len(XC.CASES)} cases, {len(XC.SEQUENCES)} sequences, {len(XC.MALFORMED)} malformed messages, 1 large case, "
          f"{len(XC.COPY_SIZES)} copy sizes, {len(XC.COPY_PAIRS)} copy pairs; {sum(sizes) / 2 ** 20:.1f} MiB over the small entries, "
          f"largest {max(sizes) / 2 ** 20:.2f} MiB; the large case {large / 2 ** 20:.1f} MiB; copies up to {MAX_COPY_BYTES / 2 ** 20:.1f} MiB")
    assert max(sizes) <= XC.MAX_CASE_BYTES and sum(sizes) <= MAX_TOTAL_BYTES
    assert XC.MAX_CASE_BYTES < large <= MAX_LARGE_BYTES
    assert sum(1 for c in entries + (XC.LARGE,) if XC.device_bytes(c) > XC.MAX_CASE_BYTES) == 1
    assert all(2 * (a + b) <= MAX_COPY_BYTES for a, b in XC.COPY_PAIRS) and 2 * max(XC.COPY_SIZES) <= MAX_COPY_BYTES
