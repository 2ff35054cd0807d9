"""The case tables of the direct exchange tests (tests/test_exchange_cases_cpu.py, tests/test_gpu_exchange_abi.py): the tile payload kernels
and the byte copies of csrc/tg_exchange.hip on raw buffers, against tests/exchange_ref.py.

CASES      (name, h, w, n_images, content): one batch of images for tg_pack_tiles / tg_unpack_tiles, with a tail of its own (tail_of).
SEQUENCES  five successive messages per rank for tg_unpack_tiles_multi, in both of its forms.
MALFORMED  messages no pack kernel writes and the unpack kernels tolerate: bad headers, ids outside the batch among valid records.
LARGE      the one case that crosses every block cap of the file (BLOCK_CAPS, read from tg_exchange.hip's launch code).
COPY_SIZES / COPY_PAIRS  byte counts for tg_copy_bytes / tg_copy_bytes2(_flag).

The template of every case is random non-zero bytes round a zero interior rectangle, like a sensor's: never all zero, so that a kernel that
compares with zero, or fills zero, is wrong on it.  "mixed" images hold, tile by tile, the template, zeros (live on the ring, not live inside),
random bytes and the template with a few bytes changed, side by side."""
import dataclasses
import functools

import numpy as np

import exchange_ref as ref

FILL = 0xA5                              # device_guard.PATTERN: what every device buffer holds before a launch
SKIP_FILL = 0x5A                         # the skipped rank's block of a destination
SHAPES = {1: (16, 16), 2: (16, 32), 4: (32, 32), 9: (48, 48), 16: (64, 64), 63: (112, 144), 64: (128, 128), 65: (80, 208), 81: (144, 144),
          256: (256, 256)}               # T -> (h, w): below one wavefront, exactly one, one plus a lane, a partly filled last group, whole groups
TALL_SHAPES = ((64, 16), (144, 112))     # H > W (SHAPES' non-square ones all have W > H)
CONTENTS = ("mixed", "none", "all", "one_first", "one_last", "one_lane63", "single_byte")
TAIL_SIZES = (0, 1, 15, 16, 17, 4089, 1 << 20)
NULL_TAIL = -17                          # tail_of: a NULL tail source with tail_bytes = 17
COPY_SIZES = (0, 1, 15, 16, 17, 31, 32, 4095, 4096, 4097, (16 << 20) - 1, 16 << 20, (16 << 20) + 21)
COPY_PAIRS = ((0, 4097), (4097, 0), (0, 0), (15, 17), (31, 1), (4095, 4096), ((16 << 20) - 1, 4097), (16, (16 << 20) + 21))
# blocks a launch is capped at, and the bytes / records one block serves without a grid-stride step (tg_exchange.hip's entry points)
BLOCK_CAPS = {"k_fill_template": (8192, 256 * 16), "k_fill_template_multi": (2048, 256 * 16), "k_scatter_tiles_multi": (4096, 16),
              "k_restore_tiles_multi": (1024, 16), "k_scatter_tiles_multi_keep": (1024, 16), "k_copy_bytes": (4096, 256 * 16)}
MAX_CASE_BYTES = 8 << 20
SEQ_KINDS = (("A", "none", "A2", "all_ff", "bad_magic"), ("all_ff", "A", "wrong_t", "A2", "none"), ("A", "none", "A2", "B", "all_ff"))
N_MESSAGES = 5


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    h: int
    w: int
    n_images: int
    content: str
    seed: int = 0

    @property
    def T(self):
        return (self.h // 16) * (self.w // 16)


@dataclasses.dataclass(frozen=True)
class Sequence:
    name: str
    h: int
    w: int
    n_images: int
    n_ranks: int
    skip_rank: int
    seed: int = 0

    @property
    def T(self):
        return (self.h // 16) * (self.w // 16)

    @property
    def stride(self):
        return (ref.capacity(self.n_images, self.h, self.w) + 15) // 16 * 16 + 48

    def kinds(self, rank):
        """The five message kinds of a rank, by its position among the ranks that are unpacked; None for the skipped rank."""
        live = [r for r in range(self.n_ranks) if r != self.skip_rank]
        return SEQ_KINDS[live.index(rank)] if rank in live else None


@dataclasses.dataclass(frozen=True)
class Malformed:
    name: str
    h: int
    w: int
    n_images: int
    what: str                            # "bad_magic", "wrong_t", "count_ff", "count_cap_plus_1", "ids"
    bad_ids: tuple = ()
    seed: int = 0

    @property
    def T(self):
        return (self.h // 16) * (self.w // 16)


def single_byte_images(T):
    """The smallest admitted image count with at least 256 tiles: every byte position of a tile is visited."""
    if T == 256:
        return 1
    n = max(5, -(-256 // T))
    return n + 1 - n % 2


def _cases():
    out = []
    add = lambda T, hw, n, content: out.append(Case(f"t{T}-{hw[0]}x{hw[1]}-n{n}-{content}", hw[0], hw[1], n, content, seed=len(out) + 1))   # noqa: E731
    for T, hw in SHAPES.items():
        for n in ((1, 3) if T == 256 else (1, 2, 5 + 2 * (T % 2))):
            add(T, hw, n, "mixed")
        add(T, hw, 2, "none")
        add(T, hw, 1 if T == 256 else 2, "all")
        add(T, hw, 2, "one_first")
        add(T, hw, 3 if T == 256 else 5, "one_last")
        if T >= 64:
            add(T, hw, 2, "one_lane63")
        add(T, hw, single_byte_images(T), "single_byte")
    for hw in TALL_SHAPES:
        T = (hw[0] // 16) * (hw[1] // 16)
        add(T, hw, 2, "mixed")
        add(T, hw, 1, "all")
    return tuple(out)


def _sequences():
    shapes = ((16, 16, 5), (48, 48, 2), (80, 208, 3), (16, 32, 7), (144, 144, 1), (64, 16, 2))
    out = []
    for n_ranks in (1, 2, 3):
        for skip in sorted({-1, 0, n_ranks // 2, n_ranks - 1}):
            h, w, n = shapes[len(out) % len(shapes)]
            out.append(Sequence(f"r{n_ranks}-skip{skip}-{h}x{w}-n{n}", h, w, n, n_ranks, skip, seed=100 + len(out)))
    out.append(Sequence("r3-skip1-16x16-n5", 16, 16, 5, 3, 1, seed=100 + len(out)))          # T = 1 with every kind of rank
    return tuple(out)


def _malformed():
    out = []
    add = lambda h, w, n, what, ids=(): out.append(Malformed(f"{h}x{w}-n{n}-{what}", h, w, n, what, tuple(ids), seed=200 + len(out)))   # noqa: E731
    # T = 1: these two ids are (int) -1 and -15 images: a signed check stores 256 and 3840 bytes in front of the destination, inside the
    # 4096 guard bytes of device_guard.Guarded.  No id here may leave that allocation under the signed check.
    add(16, 16, 5, "ids", (0xFFFFFFFF, 0xFFFFFFF1))
    for h, w, n in ((16, 32, 5), (80, 208, 1), (48, 48, 5)):
        T = (h // 16) * (w // 16)
        add(h, w, n, "ids", (n * T, n * T + 1, 0xFFFFFFFF))
    for what in ("bad_magic", "wrong_t", "count_ff", "count_cap_plus_1"):
        add(48, 48, 2, what)
        add(16, 16, 5, what)
    return tuple(out)


def template_of(h, w, seed):
    """Random non-zero bytes with a zero interior rectangle (a sensor's image: the pasted ring outside, nothing inside)."""
    rng = np.random.default_rng(7000 + seed)
    t = rng.integers(1, 256, (h, w), dtype=np.uint8)
    if h >= 48 and w >= 48:
        t[16:h - 16, 16:w - 16] = 0                                          # whole zero tiles inside whole ring tiles
    elif w >= 32:
        t[:, w // 2:] = 0
    elif h >= 32:
        t[h // 2:, :] = 0
    else:
        t[4:12, 4:12] = 0                                                    # one tile: part of it
    return t


def _tiles_view(images):
    """[n][h][w] -> a writable view [n][h/16][w/16][16][16]."""
    n, h, w = images.shape
    return images.reshape(n, h // 16, 16, w // 16, 16).transpose(0, 1, 3, 2, 4)


def _mixed(rng, tmpl, n, p=(0.4, 0.2, 0.2, 0.2)):
    """Tile by tile: the template, zeros, random bytes, the template with one to three bytes changed."""
    h, w = tmpl.shape
    img = np.broadcast_to(tmpl, (n, h, w)).copy()
    tv = _tiles_view(img)
    kind = rng.choice(4, size=tv.shape[:3], p=p)
    tv[kind == 1] = 0
    k2 = np.nonzero(kind == 2)
    tv[k2] = rng.integers(0, 256, (len(k2[0]), 16, 16), dtype=np.uint8)
    for i, a, b in zip(*np.nonzero(kind == 3)):
        m = int(rng.integers(1, 4))
        tv[i, a, b][rng.integers(0, 16, m), rng.integers(0, 16, m)] ^= rng.integers(1, 256, m, dtype=np.uint8)
    return img


def _images(rng, tmpl, n, content):
    h, w = tmpl.shape
    T, tw = (h // 16) * (w // 16), w // 16
    img = np.broadcast_to(tmpl, (n, h, w)).copy()
    tv = _tiles_view(img)

    def put(i, tile):
        tv[i, tile // tw, tile % tw] ^= rng.integers(1, 256, (16, 16), dtype=np.uint8)

    if content == "mixed":
        return _mixed(rng, tmpl, n)
    if content == "all":
        img ^= rng.integers(1, 256, img.shape, dtype=np.uint8)
    elif content == "one_first":
        put(0, 0)
    elif content == "one_last":
        put(n - 1, T - 1)
    elif content == "one_lane63":
        put(n - 1, 63)
    elif content == "single_byte":                                           # tile k: byte 37 k mod 256 (37 is odd: every position in turn)
        for k in range(n * T):
            pos = (37 * k + 11) % 256
            tv[k // T, (k % T) // tw, (k % T) % tw, pos // 16, pos % 16] ^= np.uint8((1, 128)[(k >> 1) & 1])
    else:
        assert content == "none", content
    return img


def tail_of(case):
    """(tail_bytes, tail_offset past the 16-aligned capacity) of a case; tail_bytes NULL_TAIL: a NULL source with tail_bytes 17.  The 1 MiB
    tail rides with every 8th case only."""
    i = case.seed
    sizes = TAIL_SIZES[:-1] + (NULL_TAIL,)
    return ((1 << 20) if i % 8 == 0 else sizes[i % len(sizes)]), 16 * (i % 3)


@functools.lru_cache(maxsize=4)
def build(case):
    """-> (template [h][w], images [n][h][w], tail uint8 or None, tail_offset, message buffer bytes)"""
    rng = np.random.default_rng(1000 + case.seed)
    tmpl = template_of(case.h, case.w, case.seed)
    img = _images(rng, tmpl, case.n_images, case.content)
    size, extra = tail_of(case)
    off = (ref.capacity(case.n_images, case.h, case.w) + 15) // 16 * 16 + extra
    tail = None if size == NULL_TAIL else rng.integers(0, 256, size, dtype=np.uint8)
    return tmpl, img, tail, off, off + max(size, 0) + 64


def expected_message(case, wrong=None):
    """The whole message buffer after tg_pack_tiles, records sorted by id, FILL wherever the kernel writes nothing."""
    tmpl, img, tail, off, nbytes = build(case)
    hdr, rec = ref.pack(img, tmpl, wrong)
    return ref.message(hdr, rec, nbytes, FILL, tail, off, wrong)


@functools.lru_cache(maxsize=2)
def build_sequence(seq):
    """-> (template, images[m][r] uint8 [n][h][w] (what rank r's block holds after message m), messages[m][r] uint8 [stride])
    The skipped rank's messages are valid ones of images of their own: an unpack that does not skip writes them."""
    rng = np.random.default_rng(1000 + seq.seed)
    tmpl = template_of(seq.h, seq.w, seq.seed)
    n, T, cap = seq.n_images, seq.T, ref.capacity(seq.n_images, seq.h, seq.w)
    images, messages = [], []
    first = {}
    for m in range(N_MESSAGES):
        images.append([])
        messages.append([])
        for r in range(seq.n_ranks):
            kind = (seq.kinds(r) or ("A",) * N_MESSAGES)[m]
            if kind == "A":
                img = first[r] = _mixed(rng, tmpl, n)
            elif kind == "A2":                                               # the live tiles of A again, with new bytes in half of them
                base = first.get(r)
                img = (_mixed(rng, tmpl, n) if base is None else base).copy()
                live = (_tiles_view(img) != _tiles_view(np.broadcast_to(tmpl, img.shape))).any(axis=(3, 4))
                sel = np.nonzero(live & (rng.random(live.shape) < 0.5))
                _tiles_view(img)[sel] ^= rng.integers(1, 256, (len(sel[0]), 16, 16), dtype=np.uint8)
            elif kind == "none":
                img = _images(rng, tmpl, n, "none")
            elif kind == "all_ff":
                img = _images(rng, tmpl, n, "all")
            else:                                                            # "B", "bad_magic", "wrong_t": a message of fresh images
                img = _mixed(rng, tmpl, n)
            hdr, rec = ref.pack(img, tmpl)
            if kind == "all_ff":
                assert hdr[0] == n * T
                hdr[0] = 0xFFFFFFFF                                          # above the capacity, over a full set of valid records
            elif kind == "bad_magic":
                hdr[3] ^= 0x100
            elif kind == "wrong_t":
                hdr[2] = T + 1
            rec = rec[rng.permutation(len(rec))]                             # records are in no particular order
            msg = ref.message(hdr, rec, seq.stride, FILL)
            assert 16 + rec.size <= cap < seq.stride
            messages[m].append(msg)
            images[m].append(np.broadcast_to(tmpl, img.shape).copy() if kind in ("bad_magic", "wrong_t") else img)
    return tmpl, images, messages


@functools.lru_cache(maxsize=4)
def build_malformed(mal):
    """-> (template, expected images, message bytes).  "ids": a mixed batch with the last len(bad_ids) live tiles given back to the template,
    their records replaced by records of the bad ids (random bytes) in the middle of the message."""
    rng = np.random.default_rng(1000 + mal.seed)
    tmpl = template_of(mal.h, mal.w, mal.seed)
    n, T = mal.n_images, mal.T
    img = _images(rng, tmpl, n, "all") if mal.what.startswith("count") or n * T < 16 else _mixed(rng, tmpl, n)
    hdr, rec = ref.pack(img, tmpl)
    want = img
    if mal.what == "ids":
        k = len(mal.bad_ids)
        assert len(rec) > k
        keep, rec = rec[:-k], rec[-k:].copy()
        rec[:, :4] = np.array(mal.bad_ids, np.uint32)[:, None].view(np.uint8)
        rec[:, 16:] = rng.integers(1, 256, (k, 256), dtype=np.uint8)
        mid = len(keep) // 2
        rec = np.concatenate([keep[:mid], rec, keep[mid:]])                  # the header's count names them too
        tmp_hdr = ref.header(len(keep), n, T)
        want = ref.unpack(ref.message(tmp_hdr, keep), tmpl, n, mal.h, mal.w)
    elif mal.what == "bad_magic":
        hdr[3] = 0
        want = np.broadcast_to(tmpl, img.shape).copy()
    elif mal.what == "wrong_t":
        hdr[2] = T - 1 if T > 1 else 2
        want = np.broadcast_to(tmpl, img.shape).copy()
    elif mal.what == "count_ff":
        hdr[0] = 0xFFFFFFFF
    elif mal.what == "count_cap_plus_1":
        hdr[0] = n * T + 1
    return tmpl, want, ref.message(hdr, rec, ref.capacity(n, mal.h, mal.w) + 64, FILL)


LARGE = Case("large-32x32-n33001", 32, 32, 33001, "large", seed=999)


@functools.lru_cache(maxsize=1)
def build_large():
    """-> (template, images): about 53 % of the 132 004 tiles live, one in five of them by a single byte."""
    rng = np.random.default_rng(LARGE.seed)
    tmpl = template_of(32, 32, LARGE.seed)
    n = LARGE.n_images
    img = np.broadcast_to(tmpl, (n, 32, 32)).copy()
    tv = _tiles_view(img)
    kind = rng.choice(3, size=tv.shape[:3], p=(0.47, 0.40, 0.13))
    k1 = np.nonzero(kind == 1)
    tv[k1] = rng.integers(0, 256, (len(k1[0]), 16, 16), dtype=np.uint8)
    i, a, b = np.nonzero(kind == 2)
    tv[i, a, b, rng.integers(0, 16, len(i)), rng.integers(0, 16, len(i))] ^= np.uint8(0x40)
    return tmpl, img


def live_count(tmpl, img):
    return int((_tiles_view(img) != _tiles_view(np.broadcast_to(tmpl, img.shape))).any(axis=(3, 4)).sum())


def caps_crossed(case, live):
    """Which kernels of BLOCK_CAPS take a grid-stride step on a case with `live` records (two ranks for the multi entry)."""
    nbytes, out = case.n_images * case.h * case.w, []
    for k, (blocks, per_block) in BLOCK_CAPS.items():
        work = nbytes if k.startswith("k_fill") else live
        if not k.startswith("k_copy") and work > blocks * per_block:
            out.append(k)
    return out


def single_byte_census(case):
    """For a case whose live tiles all differ from the template in one byte: ({byte positions}, {XOR values}); None otherwise."""
    tmpl, img = build(case)[:2]
    d = (_tiles_view(img) ^ _tiles_view(np.broadcast_to(tmpl, img.shape))).reshape(-1, 256)
    d = d[d.any(axis=1)]
    if len(d) == 0 or ((d != 0).sum(axis=1) != 1).any():
        return None
    return set(np.argmax(d != 0, axis=1).tolist()), set(d.max(axis=1).tolist())


def coverage_gaps(cases, sequences=None, malformed=None, copy_sizes=COPY_SIZES, copy_pairs=COPY_PAIRS):
    """What the tables lack, as tuples."""
    sequences = SEQUENCES if sequences is None else sequences
    malformed = MALFORMED if malformed is None else malformed
    gaps = []
    for T, hw in SHAPES.items():
        cs = [c for c in cases if (c.h, c.w) == hw]
        if not cs:
            gaps.append(("T", T))
            continue
        gaps += [("n_images", T, n) for n in ((1, 3) if T == 256 else (1, 2)) if not any(c.n_images == n for c in cs)]
        if T <= 81 and not any(c.n_images >= 5 and c.n_images % 2 for c in cs):
            gaps.append(("n_images", T, "odd >= 5"))
        for content in CONTENTS:
            if content == "one_lane63" and T < 64:
                continue
            if not any(c.content == content for c in cs):
                gaps.append(("content", T, content))
        for c in cs:
            if c.content == "single_byte" and single_byte_census(c) != (set(range(256)), {1, 128}):
                gaps.append(("single byte positions", T, c.name))
    nonsq = {(c.h, c.w) for c in cases if c.h != c.w}
    if len(nonsq) < 3:
        gaps.append(("non-square shapes", len(nonsq)))
    if not any(h > w for h, w in nonsq):
        gaps.append(("H > W",))
    if not any(w > h for h, w in nonsq):
        gaps.append(("W > H",))
    tails = {tail_of(c)[0] for c in cases}
    gaps += [("tail", s) for s in TAIL_SIZES + (NULL_TAIL,) if s not in tails]
    if not {0, 16, 32} <= {tail_of(c)[1] for c in cases}:
        gaps.append(("tail offsets",))
    for n_ranks in (1, 2, 3):
        for skip in {-1, 0, n_ranks // 2, n_ranks - 1}:
            if not any(s.n_ranks == n_ranks and s.skip_rank == skip for s in sequences):
                gaps.append(("sequence", n_ranks, skip))
    kinds = {k for s in sequences for r in range(s.n_ranks) for k in (s.kinds(r) or ())}
    gaps += [("sequence kind", k) for k in ("none", "all_ff", "bad_magic", "wrong_t", "A2") if k not in kinds]
    if not any(s.T == 1 for s in sequences):
        gaps.append(("sequence", "T = 1"))
    if any(s.stride <= ref.capacity(s.n_images, s.h, s.w) or s.stride % 16 for s in sequences):
        gaps.append(("sequence", "stride"))
    ids1 = {i for m in malformed if m.what == "ids" and m.T == 1 for i in m.bad_ids}
    gaps += [("malformed id", 1, i) for i in (0xFFFFFFFF, 0xFFFFFFF1) if i not in ids1]
    big = [m for m in malformed if m.what == "ids" and m.T >= 2]
    if not any({m.n_images * m.T, m.n_images * m.T + 1, 0xFFFFFFFF} <= set(m.bad_ids) for m in big):
        gaps.append(("malformed id", "T >= 2"))
    gaps += [("malformed header", w) for w in ("bad_magic", "wrong_t", "count_ff", "count_cap_plus_1") if not any(m.what == w for m in malformed)]
    cap = BLOCK_CAPS["k_copy_bytes"][0] * BLOCK_CAPS["k_copy_bytes"][1]
    gaps += [("copy size", s) for s in (0, 1, 15, 16, 17, 31, 32, 4095, 4096, 4097, cap - 1, cap, cap + 21) if s not in copy_sizes]
    if not any(a == 0 and b for a, b in copy_pairs) or not any(b == 0 and a for a, b in copy_pairs):
        gaps.append(("copy pair", "an empty member"))
    if not any(a % 16 and b % 16 for a, b in copy_pairs):
        gaps.append(("copy pair", "two tails"))
    if not any(a < cap and b < cap and a + b > cap for a, b in copy_pairs):
        gaps.append(("copy pair", "the sum crosses the cap"))
    if any(a not in copy_sizes or b not in copy_sizes for a, b in copy_pairs):
        gaps.append(("copy pair", "sizes of the list"))
    return gaps


def device_bytes(case):
    """Device memory of one run of a case without the guards: images, template, message buffer, tail, unpacked images."""
    if isinstance(case, Sequence):
        img = case.n_ranks * case.n_images * case.h * case.w
        return 2 * img + case.h * case.w + case.n_ranks * (case.stride + 4 * (1 + case.n_images * case.T))
    img = case.n_images * case.h * case.w
    if isinstance(case, Malformed):
        return img + case.h * case.w + ref.capacity(case.n_images, case.h, case.w) + 64
    if case.content == "large":                      # pack + unpack, then two ranks: messages, two destinations, one list
        cap = ref.capacity(case.n_images, case.h, case.w)
        return 2 * img + case.h * case.w + 2 * (cap + 48) + 4 * img + 2 * 4 * (1 + case.n_images * case.T)
    size, extra = tail_of(case)
    return 2 * img + case.h * case.w + ref.capacity(case.n_images, case.h, case.w) + 15 + extra + 2 * max(size, 0) + 64 + 8


CASES = _cases()
SEQUENCES = _sequences()
MALFORMED = _malformed()
