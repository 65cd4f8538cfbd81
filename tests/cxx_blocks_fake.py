"""A CPU stand-in for the two cxx listed-block entry points of libhbswizzle.so
(hb_cxx_encode_blocks_many, hb_cxx_encode_blocks) over the CPU oracle, for
testing the cxx Swizzle's Python layer without a GPU (TEST INFRASTRUCTURE
ONLY).  Every listed block is one oracle.cxx_encode(..., block_base=index,
nblocks=1); the descriptor rules of include/hbswizzle.h are enforced -- an
index of 2^32 or above among them -- so a layer that packs a list wrongly
fails here as it would on the GPU."""
import ctypes

from fake_native import FakeLib, _set

HB_EINVAL = -1
HB_EUNSUPPORTED = -4


class CxxBlocksLib(FakeLib):
    def __init__(self):
        FakeLib.__init__(self)
        self.block_calls = []      # (nfiles, [nblocks per file]) of every hb_cxx_encode_blocks_many
        self.error = b"fake"

    def hb_last_error(self, h):
        return self.error

    def hb_cxx_encode_blocks_many(self, h, pb, plen, sectors, klen, descs, n, flags, tries):
        from oracle import oracle as O
        p = int.from_bytes(bytes(pb[:plen]), "big")
        w = (p.bit_length() + 7) // 8
        C = (p.bit_length() // 8) * sectors
        files = []
        for i in range(n):
            # the struct's raw words: f_key, alpha_key, indices, nblocks, data, len, tags
            words = (ctypes.c_uint64 * 7).from_address(ctypes.addressof(descs[i]))
            fk_a, ak_a, idx_a, nb, data_a, length, tags_a = [int(x) for x in words]
            if not fk_a or not ak_a or (nb and not (idx_a and tags_a)) or (length and not data_a) or \
                    not (length == 0 if nb == 0 else (nb - 1) * C <= length <= nb * C):
                self.error = ("file %d: bad descriptor" % i).encode()
                return HB_EINVAL
            files.append((ctypes.string_at(fk_a, klen), ctypes.string_at(ak_a, klen),
                          list((ctypes.c_uint64 * nb).from_address(idx_a)) if nb else [],
                          ctypes.string_at(data_a, length) if length else b"", tags_a))
        for i, f in enumerate(files):
            if any(index >> 32 for index in f[2]):
                self.error = ("file %d: index does not fit the cxx prf's unsigned int" % i).encode()
                return HB_EUNSUPPORTED
        self.block_calls.append((int(n), [len(f[2]) for f in files]))
        total = 0
        for fk, ak, idx, data, tags_a in files:
            for k, index in enumerate(idx):
                t = O.cxx_encode(p, sectors, fk, ak, data[k * C:(k + 1) * C], block_base=index, nblocks=1)
                ctypes.memmove(tags_a + k * w, t[0].to_bytes(w, "big"), w)
                total += 1
        _set(tries, total)
        return 0


def xor_cfb128(key, iv, data, encrypt):
    """A reversible stand-in for hb_aes_cfb128 (the State's encryption)."""
    pad = (bytes(key) + bytes(iv)) * (len(data) // 16 + 1)
    return bytes(a ^ b for a, b in zip(bytes(data), pad))


def install(monkeypatch):
    """Make heartbeat_amd._native use a CxxBlocksLib; returns it."""
    from heartbeat_amd import _native, multi
    fake = CxxBlocksLib()
    monkeypatch.setattr(_native, "_lib", fake)
    monkeypatch.setattr(_native, "_ctxs", {})
    monkeypatch.setattr(_native, "aes_cfb128", xor_cfb128)
    monkeypatch.setattr(multi, "_devices", [0])
    return fake
