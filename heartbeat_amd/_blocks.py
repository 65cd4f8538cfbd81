"""The listed-block update's rules, once: what PySwizzle and the cxx Swizzle
(heartbeat.Heartbeat) check and build before hb_encode_blocks_many /
hb_cxx_encode_blocks_many run -- the order of a block list, its packing into
one descriptor, the blocks an update has to list, the blocks a byte range of a
file touches -- and the server's side, patch_tag.  The classes wrap these
under their public names; `C` is sectors x sectorsize, `n` the state's block
count."""
import numpy as np

from .exc import HeartbeatError


def sorted_blocks(blocks, index_bits):
    """[(index, bytes)] in ascending order of index; every index once and
    inside [0, 2^index_bits)."""
    out, seen = [], set()
    for index, data in blocks:
        i = int(index)
        if i < 0 or i >> index_bits:
            raise HeartbeatError("block index %d is outside [0, 2^%d)" % (i, index_bits))
        if i in seen:
            raise HeartbeatError("block index %d is listed twice" % i)
        seen.add(i)
        out.append((i, bytes(data)))
    out.sort(key=lambda t: t[0])
    return out


def pack_blocks(C, blocks):
    """(indices, packed bytes) of ascending blocks for one descriptor: all
    blocks whole but possibly the last."""
    for k, (i, data) in enumerate(blocks):
        if len(data) > C or (len(data) < C and k + 1 < len(blocks)):
            raise HeartbeatError("block %d has %d bytes, not %d" % (i, len(data), C))
    return [i for i, _ in blocks], b"".join(d for _, d in blocks)


def plan_update(C, n, blocks, length):
    """What update() checks before any GPU work: (n', ascending blocks)."""
    n = int(n)
    n_new = n if length is None else int(length) // C + 1
    if length is not None and int(length) < 0:
        raise HeartbeatError("length must not be negative")
    listed = []
    seen = set()
    for index, data in blocks:
        i = int(index)
        if i < 0 or i >= n_new:
            raise HeartbeatError("block index %d is outside the file's %d blocks" % (i, n_new))
        if i in seen:
            raise HeartbeatError("block index %d is listed twice" % i)
        seen.add(i)
        listed.append((i, bytes(data)))
    if n_new != n:
        for i in range(max(min(n, n_new) - 1, 0), n_new):
            if i not in seen:
                raise HeartbeatError("block %d must be listed when the file goes from %d to %d blocks"
                                     % (i, n, n_new))
    listed.sort(key=lambda t: t[0])
    for i, data in listed:
        if i < n_new - 1:
            if len(data) != C:
                raise HeartbeatError("block %d has %d bytes, not %d" % (i, len(data), C))
        elif length is None:
            if len(data) >= C:
                raise HeartbeatError("the last block %d has %d bytes, not fewer than %d" % (i, len(data), C))
        elif len(data) != int(length) % C:
            raise HeartbeatError("the last block %d has %d bytes, not %d" % (i, len(data), int(length) % C))
    return n_new, listed


def file_blocks(C, n, fb, changed):
    """(blocks, length) of update_file: the blocks the byte ranges touch and
    those the length rule demands, read from the file's buffer."""
    length = fb.len
    n, n_new = int(n), length // C + 1
    want = set()
    for off, nbytes in changed:
        off, nbytes = int(off), int(nbytes)
        if off < 0 or nbytes < 0 or off + nbytes > length:
            raise HeartbeatError("range (%d, %d) is outside the file's %d bytes" % (off, nbytes, length))
        if nbytes:
            want.update(range(off // C, (off + nbytes - 1) // C + 1))
    if n_new != n:
        want.update(range(max(min(n, n_new) - 1, 0), n_new))
    return [(i, fb.arr[i * C:min((i + 1) * C, length)].tobytes()) for i in sorted(want)], length


def patch_tag(Tag, tag, indices, values, nblocks=None):
    """A new Tag (of class `Tag`) of `nblocks` values (default len(tag)):
    those of `tag` with values[k] in place of block indices[k].  A tag that
    holds its fixed-width image keeps one (one numpy copy); a tag built from a
    list stays a list."""
    n_old = len(tag)
    n_new = n_old if nblocks is None else int(nblocks)
    indices = [int(i) for i in indices]
    if len(indices) != len(values):
        raise HeartbeatError("%d indices for %d values" % (len(indices), len(values)))
    for i in indices:
        if i < 0 or i >= n_new:
            raise HeartbeatError("block index %d is outside the tag's %d blocks" % (i, n_new))
    listed = set(indices)
    for i in range(n_old, n_new):
        if i not in listed:
            raise HeartbeatError("block %d is added but not listed" % i)
    if tag._sigma is None:
        w = tag._width
        if isinstance(values, Tag) and values._sigma is None and values._width == w:
            vraw = bytes(values._raw)
        else:
            vals = values.sigma if isinstance(values, Tag) else list(values)
            try:
                vraw = b"".join(int(v).to_bytes(w, "big") for v in vals)
            except OverflowError:
                raise HeartbeatError("a tag value does not fit the tag's %d bytes" % w)
        # one copy of the image: the kept values, then the listed ones over it
        keep = min(n_old, n_new) * w
        img = np.zeros(n_new * w, dtype=np.uint8)
        img[:keep] = np.frombuffer(tag._raw, dtype=np.uint8)[:keep]
        vals = np.frombuffer(vraw, dtype=np.uint8).reshape(len(indices), w) if indices else None
        rows = img.reshape(n_new, w)
        for k, i in enumerate(indices):
            rows[i] = vals[k]
        return Tag._from_raw(memoryview(img), w)
    vals = values.sigma if isinstance(values, Tag) else list(values)
    sigma = list(tag.sigma[:n_new]) + [None] * (n_new - min(n_old, n_new))
    for i, v in zip(indices, vals):
        sigma[i] = int(v)
    return Tag._from_sigma(sigma)
