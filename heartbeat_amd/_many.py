"""The Python side of the batched calls, once: descriptors in, results out.
PySwizzle.py (hb_encode_many, hb_prove_many, hb_verify_rhs_many) and Swizzle.py
(their hb_cxx_* twins) wrap these under their public names; `native` is the
entry point's name in libhbswizzle.so, `Tag` the caller's tag class."""
import ctypes

import numpy as np

from . import _native, multi
from ._filebuf import FileBuffer
from .exc import HeartbeatError


def _kb(key):
    return key.encode("latin-1") if isinstance(key, str) else bytes(key)


def _check(p, sectors):
    if p.bit_length() // 8 < 1:
        raise HeartbeatError("prime must be at least 2^8 (sector size of at least one byte)")
    if sectors < 1:
        raise HeartbeatError("sectors must be positive")


def encode_files(native, Tag, p, sectors, keys, files, open_first):
    """[(Tag, number of blocks), ...] of `files` under keys[i] = (f_key,
    alpha_key).  open_first (Swizzle.encode_files): every file is opened
    before anything else is done, and if one cannot be read, the files before
    it are consumed (left at EOF as the loop leaves them).  Without it
    (PySwizzle.encode_files) a file is opened as its descriptor is filled and
    a failure leaves the earlier files where they were."""
    p = int(p)
    sectors = int(sectors)
    files = list(files)
    keys = list(keys)
    if len(keys) != len(files):
        raise HeartbeatError("%d key pairs for %d files" % (len(keys), len(files)))
    _check(p, sectors)
    kb = [(_kb(fk), _kb(ak)) for fk, ak in keys]
    if len({len(k) for pair in kb for k in pair}) > 1:
        raise HeartbeatError("all f_keys and alpha_keys of a batch must have the same length")
    if not files:
        return []
    w = _native.width_of(p)
    C = (p.bit_length() // 8) * sectors
    fbs, outs = [], []
    try:
        descs = (_native.FileDesc * len(files))()
        if open_first:
            try:
                for file in files:
                    fbs.append(FileBuffer(file))
            except BaseException:
                for fb in fbs:
                    fb.consume()
                raise
        for i, (d, (fk, ak)) in enumerate(zip(descs, kb)):
            if not open_first:
                fbs.append(FileBuffer(files[i]))
            fb = fbs[i]
            nblocks = fb.len // C + 1
            # the tags land in the array the Tag keeps
            out = np.empty(nblocks * w, dtype=np.uint8)
            outs.append((out, nblocks))
            d.f_key, d.alpha_key = fk, ak
            d.data = fb.addr
            d.len = fb.len
            d.tags = out.ctypes.data
        ctx = multi.primary_context()
        pb = _native.be(p)
        tries = ctypes.c_uint64()
        with ctx.lock:
            ctx.check(getattr(_native.lib(), native)(ctx.h, pb, len(pb), sectors, len(kb[0][0]), descs, len(files), 0,
                                                     ctypes.byref(tries)))
        for fb in fbs:
            fb.consume()
    finally:
        for fb in fbs:
            fb.close()
    return [(Tag._from_raw(memoryview(out), w), nblocks) for out, nblocks in outs]


def encode_files_mixed(items, native, Tag, open_first):
    """[(Tag, number of blocks), ...] of `items` = (p, sectors, f_key,
    alpha_key, file) in one call of `native` (hb_encode_mixed, or
    hb_cxx_encode_mixed for the cxx Swizzle): every file under its own prime,
    sector count and key length (the files of many owners).  File handling as
    encode_files: each file from its current position to EOF and left there,
    and open_first as there."""
    keep, files = [], []
    for p, S, fk, ak, file in items:
        p, S = int(p), int(S)
        _check(p, S)
        fk, ak = _kb(fk), _kb(ak)
        if len(fk) != len(ak):
            raise HeartbeatError("f_key and alpha_key must have the same length")
        keep.append((p, S, _native.be(p), fk, ak))
        files.append(file)
    if not keep:
        return []
    n = len(keep)
    fbs, outs = [], []
    try:
        descs = (_native.EncodeMixedDesc * n)()
        if open_first:
            try:
                for file in files:
                    fbs.append(FileBuffer(file))
            except BaseException:
                for fb in fbs:
                    fb.consume()
                raise
        for i, (p, S, pb, fk, ak) in enumerate(keep):
            if not open_first:
                fbs.append(FileBuffer(files[i]))
            fb = fbs[i]
            w = _native.width_of(p)
            nblocks = fb.len // ((p.bit_length() // 8) * S) + 1
            # the tags land in the array the Tag keeps
            out = np.empty(nblocks * w, dtype=np.uint8)
            outs.append((out, nblocks, w))
            d = descs[i]
            d.p_be, d.p_len, d.sectors, d.key_len = pb, len(pb), S, len(fk)
            d.f_key, d.alpha_key = fk, ak
            d.data = fb.addr
            d.len = fb.len
            d.tags = out.ctypes.data
        ctx = multi.primary_context()
        tries = ctypes.c_uint64()
        with ctx.lock:
            ctx.check(getattr(_native.lib(), native)(ctx.h, descs, n, 0, ctypes.byref(tries)))
        for fb in fbs:
            fb.consume()
    finally:
        for fb in fbs:
            fb.close()
    return [(Tag._from_raw(memoryview(out), w), nblocks) for out, nblocks, w in outs]


def encode_blocks_many(p, sectors, items, native="hb_encode_blocks_many"):
    """The tag images of listed blocks in one call of hb_encode_blocks_many:
    `items` is a list of (f_key, alpha_key, indices, data) -- the block indices
    of one file in any order and those blocks' bytes back to back, all of them
    whole but possibly the last.  Returns one uint8 array of
    len(indices) * width(p) bytes per item, the tag values in the order of its
    indices.  All keys of a call have one length.  Runs on
    multi.primary_context()."""
    p = int(p)
    sectors = int(sectors)
    _check(p, sectors)
    keep = []
    for fk, ak, indices, data in items:
        fk, ak = _kb(fk), _kb(ak)
        idx = np.array([int(i) for i in indices], dtype=np.uint64)
        keep.append((fk, ak, idx, np.frombuffer(bytes(data), dtype=np.uint8)))
    if len({len(k) for t in keep for k in t[:2]}) > 1:
        raise HeartbeatError("all f_keys and alpha_keys of a batch must have the same length")
    if not keep:
        return []
    w = _native.width_of(p)
    descs = (_native.BlocksDesc * len(keep))()
    outs = []
    for d, (fk, ak, idx, arr) in zip(descs, keep):
        out = np.empty(len(idx) * w, dtype=np.uint8)
        outs.append(out)
        d.f_key, d.alpha_key = fk, ak
        d.indices, d.nblocks = (idx.ctypes.data if len(idx) else None), len(idx)
        d.data, d.len = (arr.ctypes.data if len(arr) else None), len(arr)
        d.tags = out.ctypes.data if len(idx) else None
    ctx = multi.primary_context()
    pb = _native.be(p)
    tries = ctypes.c_uint64()
    with ctx.lock:
        ctx.check(getattr(_native.lib(), native)(ctx.h, pb, len(pb), sectors, len(keep[0][0]), descs, len(keep), 0,
                                                 ctypes.byref(tries)))
    return outs


def prove_files(native, p, sectors, items):
    """[(mu list, sigma), ...] of `items` = (chal_key, chunks, v_max, tag,
    file).  Every file is read whole, from its start (absolute offsets, as the
    references' seek(pos) before every read: PySwizzle.py:353-355,
    shacham_waters_private.cxx:763-764), and its position is left where it
    was."""
    p = int(p)
    S = int(sectors)
    items = list(items)
    _check(p, S)
    keep = []
    for ck, chunks, v_max, tag, file in items:
        if len(tag) == 0:
            raise HeartbeatError("tag is empty")
        keep.append((_kb(ck), max(int(chunks), 0), _native.be(int(v_max)), tag, file))
    if len({len(t[0]) for t in keep}) > 1:
        raise HeartbeatError("all challenge keys of a batch must have the same length")
    if not keep:
        return []
    w = _native.width_of(p)
    n = len(keep)
    descs = (_native.ProveDesc * n)()
    out = ctypes.create_string_buffer((S + 1) * w * n)
    base = ctypes.addressof(out)
    fbs, tarrs = [], []
    try:
        for i, (ck, chunks, vmax, tag, file) in enumerate(keep):
            fb = FileBuffer(file, from_start=True)
            fbs.append(fb)
            tarr = np.frombuffer(tag.raw(p), dtype=np.uint8)
            tarrs.append(tarr)
            d = descs[i]
            d.chal_key, d.chunks = ck, chunks
            d.vmax_be, d.vmax_len = vmax, len(vmax)
            d.tags, d.ntags = tarr.ctypes.data, len(tag)
            d.data, d.len = fb.addr, fb.len
            d.mu_out = base + i * (S + 1) * w
            d.sigma_out = base + (i * (S + 1) + S) * w
        ctx = multi.primary_context()
        pb = _native.be(p)
        with ctx.lock:
            ctx.check(getattr(_native.lib(), native)(ctx.h, pb, len(pb), S, len(keep[0][0]), descs, n, 0))
    finally:
        for fb in fbs:
            fb.restore()
            fb.close()
    raw = out.raw
    res = []
    for i in range(n):
        vals = [int.from_bytes(raw[(i * (S + 1) + j) * w:(i * (S + 1) + j + 1) * w], "big") for j in range(S + 1)]
        res.append((vals[:S], vals[S]))
    return res


def verify_rhs_many(native, p, sectors, items, exact_mu):
    """The right-hand sides (ints) of `items` = (f_key, alpha_key,
    state_chunks, chal_key, chunks, v_max, mu_list) with decrypted state keys.
    exact_mu (Swizzle.verify_rhs_many): a proof has exactly `sectors` mu
    values.  Without it (PySwizzle.verify_rhs_many) it may have more, and the
    first `sectors` count."""
    p = int(p)
    S = int(sectors)
    items = list(items)
    _check(p, S)
    w = _native.width_of(p)
    keep = []
    for fk, ak, nstate, ck, chunks, v_max, mu in items:
        mu = list(mu)
        if exact_mu and len(mu) != S:
            raise HeartbeatError("proof has %d mu values, not %d" % (len(mu), S))
        if len(mu) < S:
            raise HeartbeatError("proof has fewer than %d mu values" % S)
        chunks = max(int(chunks), 0)
        keep.append((_kb(fk), _kb(ak), _kb(ck), int(nstate), chunks,
                     _native.be(int(v_max)) if chunks > 0 else b"\x01",
                     b"".join((int(m) % p).to_bytes(w, "big") for m in mu[:S])))
    if len({len(t[0]) for t in keep} | {len(t[1]) for t in keep}) > 1:
        raise HeartbeatError("all f_keys and alpha_keys of a batch must have the same length")
    if len({len(t[2]) for t in keep}) > 1:
        raise HeartbeatError("all challenge keys of a batch must have the same length")
    if not keep:
        return []
    descs = (_native.VerifyDesc * len(keep))()
    out = ctypes.create_string_buffer(w * len(keep))
    base = ctypes.addressof(out)
    for i, (fk, ak, ck, nstate, chunks, vmax, mub) in enumerate(keep):
        d = descs[i]
        d.f_key, d.alpha_key, d.chal_key = fk, ak, ck
        d.state_chunks, d.chunks = nstate, chunks
        d.vmax_be, d.vmax_len = vmax, len(vmax)
        d.mu = mub
        d.rhs_out = base + i * w
    ctx = multi.primary_context()
    pb = _native.be(p)
    with ctx.lock:
        ctx.check(getattr(_native.lib(), native)(ctx.h, pb, len(pb), S, len(keep[0][0]), len(keep[0][2]), descs,
                                                 len(keep), 0))
    raw = out.raw
    return [int.from_bytes(raw[i * w:(i + 1) * w], "big") for i in range(len(keep))]


def prove_files_mixed(items, native="hb_prove_mixed"):
    """[(mu list, sigma), ...] of `items` = (p, sectors, chal_key, chunks,
    v_max, tag, file) in one call of `native` (hb_prove_mixed, or
    hb_cxx_prove_mixed for the cxx Swizzle): every item under its own prime,
    sector count and key length (the proofs of many owners).  File handling as
    prove_files: every file read whole from its start, its position left where
    it was."""
    keep = []
    for p, S, ck, chunks, v_max, tag, file in items:
        p, S = int(p), int(S)
        _check(p, S)
        if len(tag) == 0:
            raise HeartbeatError("tag is empty")
        keep.append((p, S, _native.be(p), _kb(ck), max(int(chunks), 0), _native.be(int(v_max)), tag, file))
    if not keep:
        return []
    n = len(keep)
    descs = (_native.ProveMixedDesc * n)()
    offs, total = [], 0
    for p, S, _, _, _, _, _, _ in keep:
        offs.append(total)
        total += (S + 1) * _native.width_of(p)
    out = ctypes.create_string_buffer(max(total, 1))
    base = ctypes.addressof(out)
    fbs, tarrs = [], []
    try:
        for i, (p, S, pb, ck, chunks, vmax, tag, file) in enumerate(keep):
            w = _native.width_of(p)
            fb = FileBuffer(file, from_start=True)
            fbs.append(fb)
            tarr = np.frombuffer(tag.raw(p), dtype=np.uint8)
            tarrs.append(tarr)
            d = descs[i]
            d.p_be, d.p_len, d.sectors, d.key_len = pb, len(pb), S, len(ck)
            d.chal_key, d.chunks = ck, chunks
            d.vmax_be, d.vmax_len = vmax, len(vmax)
            d.tags, d.ntags = tarr.ctypes.data, len(tag)
            d.data, d.len = fb.addr, fb.len
            d.mu_out = base + offs[i]
            d.sigma_out = base + offs[i] + S * w
        ctx = multi.primary_context()
        with ctx.lock:
            ctx.check(getattr(_native.lib(), native)(ctx.h, descs, n, 0))
    finally:
        for fb in fbs:
            fb.restore()
            fb.close()
    raw = out.raw
    res = []
    for i, (p, S, _, _, _, _, _, _) in enumerate(keep):
        w = _native.width_of(p)
        vals = [int.from_bytes(raw[offs[i] + j * w:offs[i] + (j + 1) * w], "big") for j in range(S + 1)]
        res.append((vals[:S], vals[S]))
    return res


def verify_rhs_mixed(items, native="hb_verify_rhs_mixed", exact_mu=False):
    """The right-hand sides (ints) of `items` = (p, sectors, f_key, alpha_key,
    state_chunks, chal_key, chunks, v_max, mu_list) with decrypted state keys
    in one call of `native` (hb_verify_rhs_mixed, or hb_cxx_verify_rhs_mixed
    for the cxx Swizzle): every item under its own prime, sector count and key
    lengths.  exact_mu (Swizzle.verify_rhs_mixed): a proof has exactly
    `sectors` mu values.  Without it a proof may have more, and the first
    `sectors` count."""
    keep = []
    for p, S, fk, ak, nstate, ck, chunks, v_max, mu in items:
        p, S = int(p), int(S)
        _check(p, S)
        w = _native.width_of(p)
        mu = list(mu)
        if exact_mu and len(mu) != S:
            raise HeartbeatError("proof has %d mu values, not %d" % (len(mu), S))
        if len(mu) < S:
            raise HeartbeatError("proof has fewer than %d mu values" % S)
        fk, ak = _kb(fk), _kb(ak)
        if len(fk) != len(ak):
            raise HeartbeatError("f_key and alpha_key must have the same length")
        chunks = max(int(chunks), 0)
        keep.append((p, S, _native.be(p), fk, ak, _kb(ck), int(nstate), chunks,
                     _native.be(int(v_max)) if chunks > 0 else b"\x01",
                     b"".join((int(m) % p).to_bytes(w, "big") for m in mu[:S])))
    if not keep:
        return []
    n = len(keep)
    descs = (_native.VerifyMixedDesc * n)()
    offs, total = [], 0
    for t in keep:
        offs.append(total)
        total += _native.width_of(t[0])
    out = ctypes.create_string_buffer(max(total, 1))
    base = ctypes.addressof(out)
    for i, (p, S, pb, fk, ak, ck, nstate, chunks, vmax, mub) in enumerate(keep):
        d = descs[i]
        d.p_be, d.p_len, d.sectors, d.key_len, d.chal_key_len = pb, len(pb), S, len(fk), len(ck)
        d.f_key, d.alpha_key, d.chal_key = fk, ak, ck
        d.state_chunks, d.chunks = nstate, chunks
        d.vmax_be, d.vmax_len = vmax, len(vmax)
        d.mu = mub
        d.rhs_out = base + offs[i]
    ctx = multi.primary_context()
    with ctx.lock:
        ctx.check(getattr(_native.lib(), native)(ctx.h, descs, n, 0))
    raw = out.raw
    return [int.from_bytes(raw[offs[i]:offs[i] + _native.width_of(keep[i][0])], "big") for i in range(n)]
