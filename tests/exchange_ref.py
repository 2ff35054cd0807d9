"""The tile message of csrc/tg_exchange.hip restated in plain numpy, from the format block of include/tactile_gym_hip.h (no torch, nothing from
the package): what tests/exchange_cases.py builds its expectations with and tests/test_gpu_exchange_abi.py compares the kernels against.

  message = header {u32 count, n_images, T, magic} | count records of 272 bytes {u32 id, 12 zero bytes, 16 rows x 16 pixels}
  T = (H / 16) * (W / 16) tiles per image, tile = tr * (W / 16) + tc, id = image * T + tile
  a tile is live iff any of its 256 bytes differs from the template's

Every function takes `wrong=`: None, or the name of ONE wrong variant (WRONG) that a kernel could plausibly implement instead.  The variants
exist for tests/test_exchange_cases_cpu.py, which shows that the case table tells each of them from the right answer."""
import numpy as np

MAGIC = 0x54475431
REC = 272
WRONG = ("tiles_per_row_from_h", "last_group_dropped", "liveness_first_word_only", "no_restore", "tail_whole_words_only",
         "count_unclamped_ids_signed", "skip_rank_written")


def capacity(n_images, h, w):
    return 16 + REC * n_images * (h // 16) * (w // 16)


def tile_index(h, w, wrong=None):
    """[T][256] flat pixel indices of every tile of an [h][w] image.  tiles_per_row_from_h: the tiles per row taken from h; where that leaves
    the image the index wraps (a wrong answer only has to be wrong)."""
    assert h > 0 and w > 0 and h % 16 == 0 and w % 16 == 0
    T = (h // 16) * (w // 16)
    tw = (h if wrong == "tiles_per_row_from_h" else w) // 16
    tile = np.arange(T)
    tr, tc = tile // tw, tile % tw
    r, c = np.divmod(np.arange(256), 16)
    return (((tr[:, None] * 16 + r[None, :]) * w + tc[:, None] * 16 + c[None, :]) % (h * w)).astype(np.int64)


def header(count, n_images, T, magic=MAGIC):
    return np.array([count, n_images, T, magic], np.uint32)


def pack(images, template, wrong=None):
    """images uint8 [n][h][w], template uint8 [h][w] -> (header uint32 [4], records uint8 [count][272] sorted by id)."""
    n, h, w = images.shape
    idx = tile_index(h, w, wrong)
    T = idx.shape[0]
    tiles = images.reshape(n, h * w)[:, idx]                               # [n][T][256]
    differs = tiles != template.reshape(h * w)[idx][None]
    if wrong == "liveness_first_word_only":
        differs = differs & (np.arange(256) % 16 < 4)
    live = differs.any(axis=2)
    if wrong == "last_group_dropped":
        live[:, 64 * (T // 64):] = False
    ids = np.nonzero(live.reshape(-1))[0]
    rec = np.zeros((len(ids), REC), np.uint8)
    rec[:, :4] = ids.astype(np.uint32)[:, None].view(np.uint8)
    rec[:, 16:] = tiles.reshape(n * T, 256)[ids]
    return header(len(ids), n, T), rec


def message(hdr, records, size=None, fill=0, tail=None, tail_offset=0, wrong=None):
    """The bytes of a message buffer of `size` bytes (default: just the message) that held `fill` everywhere: header, records and, with a
    tail, its bytes at tail_offset.  tail_whole_words_only: the tail's last len % 16 bytes are dropped."""
    used = 16 + records.size
    buf = np.full(used if size is None else size, fill, np.uint8)
    buf[:16] = np.asarray(hdr, np.uint32).view(np.uint8)
    buf[16:used] = records.reshape(-1)
    if tail is not None and len(tail):
        keep = len(tail) - (len(tail) % 16 if wrong == "tail_whole_words_only" else 0)
        buf[tail_offset:tail_offset + keep] = tail[:keep]
    return buf


def sort_records(msg, count):
    """The first `count` records of a message, sorted by id: (ids uint32 [count], records uint8 [count][272])."""
    rec = np.asarray(msg[16:16 + REC * count]).reshape(count, REC)
    ids = rec[:, :4].copy().view(np.uint32).reshape(-1)
    order = np.argsort(ids, kind="stable")
    return ids[order], rec[order]


def read_records(msg, n_images, T, wrong=None):
    """(ok, ids uint32 [count], tiles uint8 [count][256]) of a message as the unpack kernels read it: a wrong magic or T is not a message
    (ok False, no records); the count is clamped to n_images * T.  count_unclamped_ids_signed: clamped only to what the buffer holds."""
    hdr = np.asarray(msg[:16]).view(np.uint32)
    if hdr[3] != MAGIC or hdr[2] != T:
        return False, np.zeros(0, np.uint32), np.zeros((0, 256), np.uint8)
    room = (len(msg) - 16) // REC
    count = min(int(hdr[0]), room if wrong == "count_unclamped_ids_signed" else n_images * T)
    assert count <= room, "the message buffer is shorter than the records its clamped count names"
    rec = np.asarray(msg[16:16 + REC * count]).reshape(count, REC)
    return True, rec[:, :4].copy().view(np.uint32).reshape(-1), rec[:, 16:]


def _accepted(ids, n_images, T, wrong):
    """Which records are stored.  Right: id < n_images * T, compared unsigned.  count_unclamped_ids_signed: (int)(id / T) < n_images."""
    if wrong == "count_unclamped_ids_signed":
        return (ids // np.uint32(T)).astype(np.int32) < n_images
    return ids.astype(np.int64) < n_images * T


def _scatter(flat, idx, ids, tiles, n_images, T, wrong):
    """flat uint8 [n_images * h * w] <- the accepted records, in message order.  An accepted id outside the batch (the signed variant only) lands
    somewhere inside it, modulo its size: a stray store has no right answer."""
    ok = _accepted(ids, n_images, T, wrong)
    hw = idx.shape[1] * T
    for i, t in zip(ids[ok].astype(np.int64), tiles[ok]):
        flat[((i // T) * hw + idx[i % T]) % flat.size] = t


def unpack(msg, template, n_images, h, w, wrong=None):
    """message bytes -> images uint8 [n_images][h][w]: the template everywhere, then the records whose id is below n_images * T."""
    idx = tile_index(h, w, wrong)
    T = idx.shape[0]
    out = np.broadcast_to(template.reshape(h * w), (n_images, h * w)).copy().reshape(-1)
    _, ids, tiles = read_records(msg, n_images, T, wrong)
    if len(ids) > 64:                                                      # the vectorised form (ids of a packed message are unique)
        ok = _accepted(ids, n_images, T, wrong)
        i = ids[ok].astype(np.int64)
        out[((i // T)[:, None] * (h * w) + idx[i % T]) % out.size] = tiles[ok]
    else:
        _scatter(out, idx, ids, tiles, n_images, T, wrong)
    return out.reshape(n_images, h, w)


class UnpackMulti:
    """tg_unpack_tiles_multi on a persistent destination uint8 [n_ranks][n_images][h][w].

    with_list False (prev_ids NULL): every rank but skip_rank gets unpack() of its message.
    with_list True: lists uint32 [n_ranks][1 + n_images * T] = {count, ids in message order}; the tiles the list names (ids below n_images * T)
    get the template back, then the new records land, then the list holds the new message's {clamped count, ids}: the destination is touched on
    the previous and the new tiles only.  A message with a wrong magic or T counts as empty.
    skip_rank's block and list are never touched.  `dst` / `lists`: the initial contents (copied)."""

    def __init__(self, template, n_ranks, n_images, h, w, skip_rank=-1, with_list=False, dst=None, lists=None, wrong=None):
        self.template, self.n_ranks, self.n, self.h, self.w = template, n_ranks, n_images, h, w
        self.skip = -1 if wrong == "skip_rank_written" else skip_rank
        self.wrong, self.with_list = wrong, with_list
        self.idx = tile_index(h, w, wrong)
        self.T = self.idx.shape[0]
        self.dst = (np.broadcast_to(template, (n_ranks, n_images, h, w)) if dst is None else dst).copy()
        self.lists = None
        if with_list:
            self.lists = (np.zeros((n_ranks, 1 + n_images * self.T), np.uint32) if lists is None else lists).copy()

    def step(self, messages):
        """messages: one uint8 array per rank (skip_rank's is not read)."""
        for r in range(self.n_ranks):
            if r == self.skip:
                continue
            if not self.with_list:
                self.dst[r] = unpack(messages[r], self.template, self.n, self.h, self.w, self.wrong)
                continue
            flat, lst, cap = self.dst[r].reshape(-1), self.lists[r], self.n * self.T
            if self.wrong != "no_restore":
                old = lst[1:1 + min(int(lst[0]), cap)]
                tmpl_tiles = self.template.reshape(-1)[self.idx]
                _scatter(flat, self.idx, old, tmpl_tiles[old.astype(np.int64) % self.T], self.n, self.T, self.wrong)
            _, ids, tiles = read_records(messages[r], self.n, self.T, self.wrong)
            ids, tiles = ids[:cap], tiles[:cap]                            # the list has room for n_images * T ids
            lst[0] = len(ids)
            lst[1:1 + len(ids)] = ids
            _scatter(flat, self.idx, ids, tiles, self.n, self.T, self.wrong)
        return self.dst

    def list_sets(self):
        """[(count, sorted ids)] per rank."""
        return [(int(l[0]), np.sort(l[1:1 + int(l[0])])) for l in self.lists]
