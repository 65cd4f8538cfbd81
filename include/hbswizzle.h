/*
 * hbswizzle.h -- C ABI of libhbswizzle.so, the MI355X (gfx950) Swizzle
 * (Shacham-Waters private PDP) hot path.
 *
 * The reference has no C ABI: its native boundary is CPython/PyCXX
 * (cxx/Swizzle.hxx) and pure Python (heartbeat/PySwizzle/PySwizzle.py).  Each
 * entry point below names the reference interface whose work it replaces.
 * The Python mirror of the reference API (heartbeat_amd.PySwizzle) binds these
 * with ctypes; INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *   - Integers crossing the ABI (primes, ranges, tags, mu, sigma) are
 *     big-endian byte strings, like Crypto.Util.number.long_to_bytes.
 *   - Tag / proof values are fixed width: hb_width(p) = ceil(bitlen(p)/8)
 *     bytes each.
 *   - Buffers are caller-owned.  A pointer flagged *_ON_DEVICE is a device
 *     pointer on the context's GPU (e.g. a torch.cuda tensor's data_ptr());
 *     otherwise it is ordinary host memory.  Nothing allocated by the library
 *     is returned to the caller.
 *   - Return value 0 = success; negative = error, message in hb_last_error().
 *     The Python layer raises HeartbeatError(message) (heartbeat/exc.py:29-35).
 *   - One context per GPU; a context must not be used by two threads at once.
 *     Calls are synchronous (they return when results are in the caller's
 *     buffers).
 *   - There is no CPU fallback: every compute entry point runs HIP kernels and
 *     fails with an error if no GPU is usable.
 */
#ifndef HBSWIZZLE_H
#define HBSWIZZLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HB_ABI_VERSION 1

/* flags */
#define HB_DATA_ON_DEVICE 1u   /* `data` is a device pointer */
#define HB_TAGS_ON_DEVICE 2u   /* `tags` / `tags_out` is a device pointer */
#define HB_ENCODE_SINGLE_PASS 4u  /* hb_encode: one-pass engine instead of the
                                     prefix-image first pass + retry pass (same
                                     tags; for A/B tests and measurements) */
#define HB_PRF_CXX 8u  /* hb_encode: the cxx Swizzle extension's PRF (cxx/prf.hxx:125-176:
                          CFB-128 over SHA256(LE32 i), <= 81 tries) and encode loop
                          (cxx/shacham_waters_private.cxx:638-702) instead of PySwizzle's
                          KeyedPRF; needs ByteCount(p) % 16 == 0 (the cxx API's 1024-bit
                          primes, 256-bit primes).  Tags differ from PySwizzle's.
                          Parity unpinned (Crypto++ absent). */

#define HB_ASYNC 16u  /* hb_encode with device-resident data and tags: return once the
                        encode kernels are enqueued on the context's stream (the
                        prologue -- alpha PRF, MFMA fragments -- still completes
                        first); hb_ctx_wait, or the context's next call, completes
                        it.  With hb_ctx_set_stream the kernels run on the
                        caller's stream ("an async variant takes a
                        hipStream_t"). */

#define HB_HOST_REGISTER 32u  /* hb_encode with host buffers: page-lock the file bytes
                                 read-only (hipHostRegisterReadOnly) and the host tag
                                 buffer for writing, in page-aligned windows of
                                 256 MiB pinned ahead of the copies by helper
                                 threads, and DMA the chunks straight from / into
                                 them (each window unpinned once its copies are
                                 done), instead of the runtime's pageable staging.
                                 For read-only mappings of files (the reference's
                                 file object, PySwizzle.py:299) and other large host
                                 buffers (files under 32 MiB are copied pageable:
                                 the windows would cost more than they save); a window that cannot be registered (e.g.
                                 already registered by the caller) is copied as is.
                                 Same tags. */

/* error codes */
#define HB_OK 0
#define HB_EINVAL -1
#define HB_EHIP -2
#define HB_ENOMEM -3
#define HB_EUNSUPPORTED -4

typedef struct hb_ctx hb_ctx;

int hb_abi_version(void);

/* Build properties.  HB_BUILD_EXPERIMENT: an A/B experiment build
 * (scripts/build_variant.sh) whose HB_EXP_* switches may emit wrong tags; the
 * Python package refuses such a library unless HB_LIB_PATH names it.
 * HB_BUILD_TEST_SWITCHES: HB_ENABLE_TEST_SWITCHES=1 is set in this process's
 * environment, so contexts created now honour the A/B and test switches
 * (hb_test_switches) -- never set for measurements. */
#define HB_BUILD_EXPERIMENT 1
#define HB_BUILD_TEST_SWITCHES 2
int hb_build_flags(void);

/* Provenance: hex SHA-256 of every source file of this library
 * (heartbeat_amd/csrc, this header) and of its compiler flags, as computed by
 * heartbeat_amd/build_id.py at build time; and those flags.  The Python
 * package refuses a library whose id does not match the tree it sits in. */
const char *hb_build_id(void);
const char *hb_build_flags_string(void);

/* The A/B and test switches (environment variables) a
 * context created now would honour, as a bit mask (HB_SW_*).  All of them
 * are ignored -- mask 0 -- unless HB_ENABLE_TEST_SWITCHES=1 is set when the
 * context is created; a context reads that gate once, at creation. */
#define HB_SW_NO_QUAD 1u
#define HB_SW_NO_MFMA 2u
#define HB_SW_MFMA_SECTOR_LOADS 4u
#define HB_SW_MFMA_LINE32 8u
#define HB_SW_MFMA_MIN_S 16u
#define HB_SW_NO_EARLY_LIST 32u
#define HB_SW_RETRY_CAP 64u
#define HB_SW_PROVE_BATCH 128u
#define HB_SW_TRACE_PHASES 256u
#define HB_SW_HOST_WINDOWS 512u   /* HB_HOST_WINDOW_MIB / HB_HOST_AHEAD: HB_HOST_REGISTER geometry */
#define HB_SW_NO_PROVE_GATHER 1024u  /* HB_NO_PROVE_GATHER: device proves sum straight from the file */
#define HB_SW_SUMS_ON_DEVICE 2048u   /* HB_SUMS_ON_DEVICE: weighted sums land in device memory + a D2H copy */
#define HB_SW_NO_PROVE_PLACE 4096u   /* HB_NO_PROVE_PLACE: prove PRF waves take jobs from the queue, not by SIMD */
#define HB_SW_NO_PROVE_FUSE 8192u    /* HB_NO_PROVE_FUSE: device proves sum in a second launch (hb_wsum_kernel) */
#define HB_SW_SYNC_WAIT 16384u       /* HB_SYNC_WAIT: a fused prove waits for its stream instead of polling its token */
#define HB_SW_NO_VERIFY_FUSE 32768u  /* HB_NO_VERIFY_FUSE: verify as a launch sequence (PRFs, mont, hb_wsum_kernel) */
#define HB_SW_NO_SMALL_ENCODE 65536u /* HB_NO_SMALL_ENCODE: the two-pass engine for small inputs too */
#define HB_SW_NO_PROVE_UPLOAD 131072u /* HB_NO_PROVE_UPLOAD: small host files are gathered on the host, not uploaded */
#define HB_SW_MID_BLOCKS 262144u     /* HB_MID_BLOCKS=n: up to n blocks per launch (default 17 x 256 x #CUs; 16 x for primes above 256 bits) take the queued quad-PRF + MAC path */
#define HB_SW_NO_WIDE 524288u       /* HB_NO_WIDE: primes above 256 bits keep the MAC inside the PRF kernels (VALU) instead of the split F-only passes + MFMA MAC (hb_wmac_kernel) */
#define HB_SW_WMAC_WPE 1048576u     /* HB_WMAC_WPE=1|3|5: hb_wmac_kernel built for another waves-per-SIMD bound (1: the compiler's choice) */
#define HB_SW_WIDE_SYNC_ALPHA 2097152u /* HB_WIDE_SYNC_ALPHA: the split encode computes alpha and its digit table on the compute stream, before the PRF passes, instead of beside them */
#define HB_SW_QCHUNK 4194304u       /* HB_QCHUNK=n: jobs per queue refill in the encode engines (default 256 up to 256-bit primes, 64 above; rounded up to a multiple of 64) */
#define HB_SW_DIGEST_CACHE 8388608u  /* HB_DIGEST_CACHE_MIB=n: cap of the context's digest table in MiB for this call, over hb_ctx_set_digest_cache's (0: no table) */
#define HB_SW_BATCH_BLOCKS 16777216u  /* HB_TEST_BATCH_BLOCKS=n: hb_encode_many and hb_cxx_encode_many put at most n blocks into one group of launches, and files of more than n blocks go to the single-file encode; hb_encode_blocks_many and hb_cxx_encode_blocks_many put at most n listed blocks into one group and continue a longer list in the next */
#define HB_SW_BATCH_CHUNKS 33554432u  /* HB_TEST_BATCH_CHUNKS=n: hb_verify_rhs_many, hb_prove_many and their cxx counterparts put at most n challenge indices into one group of launches, and proofs of more than n chunks go to the single verify / prove */
uint32_t hb_test_switches(void);

/* Number of visible HIP devices (multi-GPU sharding of encode / prove opens
 * one context per device; contexts fail on non-gfx950 devices). */
int hb_device_count(int *n);

/* PCI bus id ("dddd:bb:dd.f", NUL-terminated, n >= 16) of HIP device
 * `device`: tells physically distinct GPUs apart (bench.py's
 * distinct_devices) whatever ordinal remapping a launcher applies. */
int hb_device_pci_bus_id(int device, char *out, size_t n);

/* Open a context on HIP device `device`.  Replaces nothing in the reference
 * (it runs on the host only); the reference's per-call state lives in
 * PySwizzle objects (PySwizzle.py:233-255). */
int hb_ctx_create(int device, hb_ctx **out);
void hb_ctx_destroy(hb_ctx *ctx);
/* Message of the last error on this context (or of the last failed
 * hb_ctx_create when ctx is NULL). */
const char *hb_last_error(const hb_ctx *ctx);

/* Compute units of the context's device (the small-input encode and the
 * prove size their launches by it; tests place inputs at those limits).
 * Replaces nothing in the reference. */
int hb_ctx_num_cus(const hb_ctx *ctx, int *out);

/* Enqueue this context's kernels on `stream` (a hipStream_t of the
 * context's device, e.g. torch.cuda.current_stream().cuda_stream), or on the
 * context's own stream again with NULL.  Waits for the work already enqueued
 * on the previous stream. */
int hb_ctx_set_stream(hb_ctx *ctx, void *stream);

/* Complete an HB_ASYNC hb_encode: wait for its kernels, check its PRF
 * counters.  Returns the status of the async encodes completed since the last
 * hb_ctx_wait -- the FIRST failure among them, 0 if none failed -- and
 * *tries_out (may be NULL) receives their PRF tries.  Read the tags after
 * this call. */
int hb_ctx_wait(hb_ctx *ctx, uint64_t *tries_out);

/* Load the GPU code of the kernels that encodes and proves with a prime of
 * `prime_bits` bits launch, ahead of the first such call (the HIP runtime
 * otherwise loads a kernel translation unit's code object inside its first
 * launch: ~5 ms for the 256-bit unit).  Optional; replaces nothing in the
 * reference (setup, like creating a library handle). */
int hb_ctx_prepare(hb_ctx *ctx, uint32_t prime_bits);

/* The digest table of the two-pass encode.  Every block's PRF input is
 * SHA256(str(block index)) (heartbeat/util.py:91), which depends on the index
 * alone -- not on the file, the keys or the prime -- so a context keeps the
 * digests of one contiguous index range on the device, 32 bytes per block
 * (1/16 of the file at S = 16 with 32-byte sectors, as large as the file at
 * S = 1): the first encode of a range stores them while it hashes, later
 * encodes inside the range load them instead.  The cxx prf, the single-pass
 * encode and the small / mid-size paths do not use it.
 * hb_ctx_set_digest_cache: the most bytes the table may take (default 8 GiB:
 * 2^28 indices); a table larger than that is freed, and 0 turns the feature
 * off.  A table that does not fit, or cannot be allocated, only means that
 * the encode hashes.  Replaces nothing in the reference.
 * hb_ctx_digest_cache_info: the valid index range [*lo, *hi), the bytes
 * allocated and what the last hb_encode did (0 hashed without the table,
 * 1 hashed and stored, 2 loaded); any pointer may be NULL. */
int hb_ctx_set_digest_cache(hb_ctx *ctx, uint64_t max_bytes);
int hb_ctx_digest_cache_info(hb_ctx *ctx, uint64_t *lo, uint64_t *hi, uint64_t *bytes, uint32_t *last_mode);

/* ceil(bitlen(p)/8): width of every tag / mu / sigma value. */
size_t hb_width(const uint8_t *p_be, size_t p_len);

/* Batched KeyedPRF.eval.
 * Replaces heartbeat/util.py:83-96 (KeyedPRF.eval) and, for the cxx twin's
 * callers, cxx/prf.hxx:125-145 (prf::evaluate) -- with PySwizzle semantics.
 * out[i] = KeyedPRF(key, range).eval(xs[i]), written big-endian with
 * ceil(bitlen(range)/8) bytes each.  key: 16, 24 or 32 bytes (AES-128/192/256).
 * xs and out are host buffers. */
int hb_prf_eval(hb_ctx *ctx, const uint8_t *key, size_t key_len,
                const uint8_t *range_be, size_t range_len,
                const uint64_t *xs, size_t n, uint8_t *out);

/* KeyedPRF.eval over caller-hashed inputs.
 * Replaces heartbeat/util.py:83-96 for inputs hb_prf_eval cannot take: the
 * reference hashes str(x) of ANY Python int (util.py:91), negative and wider
 * than 64 bits included.  digests: n x 32 bytes, digest i = SHA256(str(x_i));
 * out as hb_prf_eval. */
int hb_prf_eval_digests(hb_ctx *ctx, const uint8_t *key, size_t key_len,
                        const uint8_t *range_be, size_t range_len,
                        const uint8_t *digests, size_t n, uint8_t *out);

/* Merkle chunk positions.
 * Replaces the KeyedPRF call of heartbeat/Merkle/Merkle.py:497-504
 * (MerkleHelper.get_chunk_hash): with chunk = min(chunksz, filesz),
 *   offsets[i] = KeyedPRF(seed_i, filesz - chunk + 1).eval(0)
 * for nseeds seeds of seed_len (16, 24 or 32) bytes each (every seed is its
 * own AES key).  seeds and offsets are host buffers. */
int hb_merkle_offsets(hb_ctx *ctx, const uint8_t *seeds, size_t seed_len, uint64_t nseeds,
                      uint64_t filesz, uint64_t chunksz, uint64_t *offsets);

/* Merkle chunk leaves.
 * Replaces the HMAC loop of heartbeat/Merkle/Merkle.py:505-515:
 *   digests[i] = HMAC-SHA256(seed_i, data[offsets[i] : offsets[i] + chunk_len])
 * over a DEVICE-resident data buffer of len bytes (every chunk must lie
 * inside it); one GPU lane hashes one chunk (a serial SHA-256 stream).
 * seed_len: 1..64 bytes.  seeds, offsets (host) and digests (host,
 * nseeds * 32 bytes). */
int hb_merkle_chunk_hmacs(hb_ctx *ctx, const uint8_t *seeds, size_t seed_len, uint64_t nseeds,
                          const uint8_t *data_dev, uint64_t len, const uint64_t *offsets,
                          uint64_t chunk_len, uint8_t *digests);

/* Merkle encode of many files in one call.
 * Replaces heartbeat/Merkle/Merkle.py:355-364 (Merkle.encode's seed chain,
 * its n get_chunk_hash calls and MerkleTree.build) for nfiles files, each
 * under its own key, seed, n and chunk size (one owner's files, or many
 * owners').  With chunk = min(chunksz, filesz) (Merkle.py:500-501),
 * s_1 = HMAC-SHA256(key, seed), s_{k+1} = HMAC-SHA256(key, s_k):
 *   offsets_out[k] = KeyedPRF(s_{k+1}, filesz - chunk + 1).eval(0)
 *   leaves_out[k]  = HMAC-SHA256(s_{k+1}, data[offsets_out[k] : +chunk])
 *   nodes_out      = the tree's (2 << order) nodes of 32 bytes each in the
 *                    reference's numbering (MerkleTree.py:29-36), node
 *                    2^order - 1 + k = SHA-256(leaf k || decimal(k)), empty
 *                    slots (leaf slots >= n, the last entry) all zero;
 *                    order = 0 for n = 1, else the bit length of n - 1.
 * Three launches serve the whole batch: the seed chains (a lane per file; on
 * the host for a few files), the leaves (a lane per leaf) and the trees (a
 * workgroup per file).  A host file of more than max(2 n chunk, 8 MiB) bytes
 * is not uploaded: its positions come back first and only its chunks go up.
 * flags: HB_DATA_ON_DEVICE (every `data` is a device pointer), and at most
 * one of HB_MERKLE_CHAIN_HOST / HB_MERKLE_CHAIN_DEVICE to force where the
 * chains run; anything else returns HB_EINVAL.  Every descriptor is checked
 * before the first launch: 1 <= n <= 65536, filesz <= len ("chunk past the
 * end of the data"), no NULL buffer; a range filesz - chunk + 1 of 2^64 is
 * HB_EUNSUPPORTED.  nfiles = 0 is a no-op.  After a call in which no file was
 * gathered, hb_last_kernel_phases reports its four phases: the chains (or the
 * upload of the host's seeds), the leaves, the trees, the copies back. */
#define HB_MERKLE_CHAIN_HOST 64u
#define HB_MERKLE_CHAIN_DEVICE 128u
#define HB_MERKLE_MAX_N 65536u
typedef struct hb_merkle_encode_desc {
    const uint8_t *key;      /* the owner's HMAC key, key_len bytes (may be NULL when key_len == 0) */
    uint64_t key_len;
    const uint8_t *seed;     /* the state seed, seed_len bytes of any length */
    uint64_t seed_len;
    uint64_t n;              /* leaves (challenges) */
    uint64_t filesz;         /* the size the positions are drawn for; <= len */
    uint64_t chunksz;
    const uint8_t *data;     /* host, or device with HB_DATA_ON_DEVICE; may be NULL when filesz == 0 */
    uint64_t len;            /* readable bytes at data */
    uint8_t *nodes_out;      /* host, (2 << order) * 32 bytes */
    uint8_t *leaves_out;     /* host, n * 32 bytes, or NULL */
    uint64_t *offsets_out;   /* host, n positions, or NULL */
} hb_merkle_encode_desc;
int hb_merkle_encode_many(hb_ctx *ctx, const hb_merkle_encode_desc *files, uint64_t nfiles,
                          uint32_t flags);

/* Merkle leaves of many proofs in one call (the prove side, Merkle.py:399-403).
 * Proof i, under its own seed (16, 24 or 32 bytes), file and range:
 *   offset_out = KeyedPRF(seed, filesz - chunk + 1).eval(0), chunk = min(chunksz, filesz)
 *   leaf_out   = HMAC-SHA256(seed, data[offset : offset + chunk])   (32 bytes)
 * A lane per proof.  Host files are uploaded or gathered as in
 * hb_merkle_encode_many (n = 1).  flags: HB_DATA_ON_DEVICE or 0.  Checked
 * before the first launch: filesz <= len, the seed length, no NULL buffer
 * (offset_out may be NULL). */
typedef struct hb_merkle_leaf_desc {
    const uint8_t *seed;
    uint64_t seed_len;
    uint64_t filesz;
    uint64_t chunksz;
    const uint8_t *data;     /* host, or device with HB_DATA_ON_DEVICE; may be NULL when filesz == 0 */
    uint64_t len;
    uint8_t *leaf_out;
    uint64_t *offset_out;
} hb_merkle_leaf_desc;
int hb_merkle_leaves_many(hb_ctx *ctx, const hb_merkle_leaf_desc *proofs, uint64_t nproofs,
                          uint32_t flags);

/* OneHash challenges of many files in one call.
 * Replaces heartbeat/OneHash/OneHash.py:92-110 (generate_challenges: its
 * generate_seeds chain and its num meet_challenge calls) for nfiles files,
 * each under its own secret, first seed, num and blocks (pick_blocks draws
 * from Python's generator and stays with the caller).  With
 * c = min(1024, len / 10), s_0 = s0 and s_{k+1} = SHA-256(s_k || secret):
 *   seeds_out[job]     = s_k                                       (32 bytes)
 *   responses_out[job] = SHA-256(part(blocks[k]) || s_k)           (32 bytes)
 * for job = (the num of the files before) + k, where part(b) is
 * data[b : b + c] when b <= len - c, and otherwise, with a = b - (len - c),
 * data[b : min(b + a, len)] || data[0 : c - a]: the reference's first read
 * stops at the end of the file, so the part is shorter than c when a > c / 2.
 * Two launches serve the whole batch: the seed chains (a lane per file; on
 * the host for a few files, and always for a secret of more than 87 bytes)
 * and the responses (a lane per job).  A host file of more than
 * max(2 * num * 1024, 8 MiB) bytes is not uploaded: only its jobs' segments
 * go up.
 * flags: HB_DATA_ON_DEVICE (every `data` is a device pointer), and at most
 * one of HB_ONEHASH_CHAIN_HOST / HB_ONEHASH_CHAIN_DEVICE to force where the
 * chains run; anything else returns HB_EINVAL.  Every descriptor is checked
 * before the first launch: every block < len, no NULL buffer (secret may be
 * NULL when secret_len == 0, data when len == 0, blocks when num == 0); more
 * than 2^31 jobs in all is HB_EUNSUPPORTED.  nfiles = 0 is a no-op. */
#define HB_ONEHASH_CHAIN_HOST 64u
#define HB_ONEHASH_CHAIN_DEVICE 128u
#define HB_ONEHASH_MAX_SEED_LEN 64u
typedef struct hb_onehash_gen_desc {
    const uint8_t *data;      /* host, or device with HB_DATA_ON_DEVICE; may be NULL when len == 0 */
    uint64_t len;             /* the file's size */
    const uint8_t *s0;        /* the first seed, 32 bytes: SHA-256 of the root seed */
    const uint8_t *secret;    /* secret_len bytes of any length */
    uint64_t secret_len;
    uint64_t num;             /* challenges */
    const uint64_t *blocks;   /* host, num positions, each < len */
} hb_onehash_gen_desc;
int hb_onehash_generate_many(hb_ctx *ctx, const hb_onehash_gen_desc *files, uint64_t nfiles,
                             uint8_t *seeds_out, uint8_t *responses_out, uint32_t flags);

/* OneHash responses of many challenges in one call (meet_challenge,
 * OneHash.py:112-138).  Job j, over file jobs[j].file:
 *   responses_out[j] = SHA-256(part(block) || seed[0 : seed_len])  (32 bytes)
 * with part() as in hb_onehash_generate_many.  A lane per job; the jobs may
 * name the files in any order, and a file is uploaded (or gathered) once
 * however many jobs read it, by the same threshold with num = the file's
 * jobs.  flags: HB_DATA_ON_DEVICE or 0.  Checked before the first launch:
 * file < nfiles, block < the file's len, seed_len <= 64, no NULL buffer.
 * njobs = 0 is a no-op. */
typedef struct hb_onehash_file {
    const uint8_t *data;      /* host, or device with HB_DATA_ON_DEVICE; may be NULL when len == 0 */
    uint64_t len;
} hb_onehash_file;
typedef struct hb_onehash_job {
    uint64_t file;            /* index into files */
    uint64_t block;
    uint64_t seed_len;        /* 0..64 */
    uint8_t seed[64];
} hb_onehash_job;
int hb_onehash_meet_many(hb_ctx *ctx, const hb_onehash_file *files, uint64_t nfiles,
                         const hb_onehash_job *jobs, uint64_t njobs, uint8_t *responses_out,
                         uint32_t flags);

/* Jobs from which heartbeat_amd.OneHash sends a call to the GPU (below, its
 * host path is faster): the measured crossover, hb_onehash_host.hpp. */
uint64_t hb_onehash_device_min_jobs(void);

/* The positions of OneHash.pick_blocks for many files in one launch
 * (OneHash.py:170-189): file i's num draws of randint(0, len - 1) from
 * Python's generator after random.seed(root_seed), bit for bit (CPython's
 * MT19937, seed version 2).  The caller makes the key from the root seed: for
 * str (UTF-8), bytes and bytearray n = int.from_bytes(a + sha512(a).digest(),
 * "big"), for int n = abs(a); key = the 32-bit words of n, least significant
 * first, [0] for n = 0.  The device never sees the root seed.
 *   blocks_out[k] = the k-th position                         (num values)
 *   state_out     = what random.getstate() holds afterwards: mt[0..623] and
 *                   the index (the twist is lazy: 624 after exactly 624 * m
 *                   words)                                     (625 words)
 * A wave per file.  flags: 0.  Every descriptor is checked before the launch
 * and nothing is written when one fails (hb_last_error names the file):
 * len == 0 with num > 0, key_words == 0, a NULL key, and a NULL blocks_out
 * with num > 0 are HB_EINVAL; key_words above HB_ONEHASH_MAX_KEY_WORDS and
 * more than 2^31 jobs in all are HB_EUNSUPPORTED.  nfiles = 0 is a no-op. */
#define HB_ONEHASH_MAX_KEY_WORDS 1024u      /* seeds of up to 4032 bytes */
typedef struct hb_onehash_draw_desc {
    uint64_t len;            /* positions are drawn in [0, len); >= 1 when num > 0 */
    const uint32_t *key;     /* key_words words, least significant first */
    uint64_t key_words;      /* 1 .. HB_ONEHASH_MAX_KEY_WORDS */
    uint64_t num;
    uint64_t *blocks_out;    /* host, num values; may be NULL when num == 0 */
    uint32_t *state_out;     /* host, 625 words: mt[0..623], index; or NULL */
} hb_onehash_draw_desc;
int hb_onehash_pick_blocks_many(hb_ctx *ctx, const hb_onehash_draw_desc *files,
                                uint64_t nfiles, uint32_t flags);

/* hb_onehash_generate_many with the positions drawn on the device: file i's
 * blocks are those of hb_onehash_pick_blocks_many for (len, key, num).  One
 * draw launch, then the chain and response launches; the positions stay in
 * device memory between them and come back with the seeds and responses.
 * For a host file above the upload threshold, whose segments the host
 * gathers, the positions come down before the gather.  flags and checks are
 * those of hb_onehash_generate_many (without its block check) and of
 * hb_onehash_pick_blocks_many. */
typedef struct hb_onehash_drawn_desc {
    const uint8_t *data;      /* host, or device with HB_DATA_ON_DEVICE; may be NULL when len == 0 */
    uint64_t len;             /* the file's size: positions are drawn in [0, len) */
    const uint8_t *s0;        /* the first seed, 32 bytes: SHA-256 of the root seed */
    const uint8_t *secret;    /* secret_len bytes of any length */
    uint64_t secret_len;
    uint64_t num;             /* challenges */
    const uint32_t *key;      /* key_words words, least significant first */
    uint64_t key_words;       /* 1 .. HB_ONEHASH_MAX_KEY_WORDS */
    uint64_t *blocks_out;     /* host, num values; may be NULL when num == 0 */
    uint32_t *state_out;      /* host, 625 words, or NULL */
} hb_onehash_drawn_desc;
int hb_onehash_generate_drawn_many(hb_ctx *ctx, const hb_onehash_drawn_desc *files, uint64_t nfiles,
                                   uint8_t *seeds_out, uint8_t *responses_out, uint32_t flags);

/* Jobs from which heartbeat_amd.OneHash draws the positions of a GPU call of
 * one file on the device when the caller does not say: the measured
 * crossover, hb_onehash_host.hpp.  Calls of several files draw on the device
 * only when asked to.  0: every call only when asked to. */
uint64_t hb_onehash_draw_device_min_jobs(void);

/* Swizzle encode of a run of blocks.
 * Replaces heartbeat/PySwizzle/PySwizzle.py:296-309 (the encode loop) and
 * cxx/shacham_waters_private.cxx:672-697.  For k in [0, nblocks):
 *   tags[k] = (F(block_base + k) + sum_j alpha(j) * m_kj) mod p
 * with F = KeyedPRF(f_key, p), alpha = KeyedPRF(alpha_key, p), sector size
 * ss = bitlen(p)/8, block size C = sectors*ss and m_kj the big-endian integer
 * of data[k*C + j*ss : min(k*C + (j+1)*ss, len)] (0 when empty; sectors after
 * the first short one contribute 0, PySwizzle.py:304-306).
 * A whole-file PySwizzle.encode is block_base = 0, nblocks = len/C + 1
 * (hb_block_count); shards of a file pass their first block index as
 * block_base and only their own bytes.
 * tags: nblocks * hb_width(p) bytes.  *tries_out (may be NULL) receives the
 * total number of PRF tries spent on the F values (>= nblocks). */
int hb_encode(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
              const uint8_t *f_key, const uint8_t *alpha_key, size_t key_len,
              uint64_t block_base, const uint8_t *data, uint64_t len,
              uint64_t nblocks, uint8_t *tags, uint32_t flags,
              uint64_t *tries_out);

/* Swizzle encode of many whole files, each under its own keys, in one call.
 * Replaces a caller's loop over heartbeat/PySwizzle/PySwizzle.py:279-311
 * (PySwizzle.encode draws a fresh f_key and alpha_key per file, :281): file
 * i's tags are exactly what hb_encode writes for it with block_base = 0 and
 * nblocks = hb_block_count(p, sectors, len) (a file with len == 0 has one
 * block, tag = F(0)), PySwizzle's KeyedPRF.  One prime, one `sectors` and one
 * key_len (16, 24 or 32) for the batch; keys, data, length and tag buffer per
 * file.  A small file is bound by the latency of its longest PRF rejection
 * chain, not by throughput: the batch runs the chains of all files side by
 * side -- one PRF launch and one MAC launch per group of files (the runtime
 * splits a batch whose device scratch would pass its cap) -- and files with
 * more blocks than that path takes go through the single-file encode inside
 * the same call, so any mix of sizes is accepted.
 * flags: HB_DATA_ON_DEVICE / HB_TAGS_ON_DEVICE (device pointers of any
 * alignment); HB_HOST_REGISTER is ignored; HB_PRF_CXX, HB_ASYNC and
 * HB_ENCODE_SINGLE_PASS return HB_EUNSUPPORTED.  Host files go up in one copy
 * from a pinned staging buffer, the tags come back in one.  nfiles == 0
 * returns HB_OK.  *tries_out (may be NULL) receives the sum of the files' F
 * tries: what nfiles hb_encode calls report in total. */
typedef struct hb_file_desc {
    const uint8_t *f_key, *alpha_key;  /* key_len bytes each */
    const uint8_t *data;               /* host, or device with HB_DATA_ON_DEVICE; may be NULL when len == 0 */
    uint64_t len;
    uint8_t *tags;                     /* hb_block_count(p, sectors, len) * hb_width(p) bytes;
                                          host, or device with HB_TAGS_ON_DEVICE */
} hb_file_desc;

int hb_encode_many(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
                   size_t key_len, const hb_file_desc *files, uint64_t nfiles,
                   uint32_t flags, uint64_t *tries_out);

/* Swizzle tags of listed blocks: the blocks an edit or an append changed, of
 * one file or of many files each under its own keys, in one call.
 * Replaces a caller's loop over the body of heartbeat/PySwizzle/PySwizzle.py:296-309
 * for chosen values of i: tag_i = F(i) + sum_j alpha_j m_ij mod p depends on
 * nothing but block i and its index, so a changed block needs neither the rest
 * of the file nor fresh keys.  tags[k] of a file are exactly the bytes that
 * hb_encode writes for block_base = indices[k], data + k*C, len_k =
 * min(C, len - k*C) and nblocks = 1, with C = sectors * ss: the listed blocks
 * lie back to back at `data`, all of them C bytes but possibly the last, whose
 * short sector is the big-endian integer of the bytes it has, whose later
 * sectors are 0 (PySwizzle.py:304-306), and which, when empty, gives
 * tag = F(index).  indices may come in any order and may repeat; every value up
 * to 2^64 - 1 is accepted (F hashes the index's decimal string).  One prime,
 * one `sectors` and one key_len (16, 24 or 32) for the batch.  A group of lists
 * is one copy up (indices, key schedules and host data together), one PRF
 * launch (F(indices[k]) of every listed block and alpha_j of every file, each
 * under its file's schedules), hb_encode_many's MAC launch over the packed
 * blocks, and one copy down; the runtime splits a call, and a single list,
 * whose device scratch would pass the batches' cap ($HB_TEST_BATCH_BLOCKS: at
 * that many listed blocks).
 * flags: HB_DATA_ON_DEVICE / HB_TAGS_ON_DEVICE (device pointers of any
 * alignment); any other flag, HB_PRF_CXX and HB_ASYNC among them, returns
 * HB_EUNSUPPORTED.  Every descriptor is checked before any GPU work and
 * hb_last_error names the file ("file 3: ..."): a NULL key, NULL indices or
 * tags with nblocks > 0, a len outside [(nblocks - 1) * C, nblocks * C] (0 for
 * nblocks == 0), or NULL data with len > 0 returns HB_EINVAL and no tag buffer
 * is written.  nfiles == 0 and nblocks == 0 are no-ops.  *tries_out (may be
 * NULL) receives the sum of the listed blocks' F tries: what those single
 * hb_encode calls report in total. */
typedef struct hb_blocks_desc {
    const uint8_t *f_key, *alpha_key;  /* key_len bytes each */
    const uint64_t *indices;           /* host, nblocks block indices: any order, repeats allowed */
    uint64_t nblocks;
    const uint8_t *data;               /* listed block k at data + k*C; host, or device with HB_DATA_ON_DEVICE */
    uint64_t len;                      /* (nblocks-1)*C <= len <= nblocks*C: only the LAST listed block may be short */
    uint8_t *tags;                     /* nblocks * hb_width(p) bytes; host, or device with HB_TAGS_ON_DEVICE */
} hb_blocks_desc;

int hb_encode_blocks_many(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
                          size_t key_len, const hb_blocks_desc *files, uint64_t nfiles,
                          uint32_t flags, uint64_t *tries_out);

/* hb_encode_blocks_many for one file (nfiles = 1; errors read "file 0: ..."). */
int hb_encode_blocks(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
                     const uint8_t *f_key, const uint8_t *alpha_key, size_t key_len,
                     const uint64_t *indices, uint64_t nblocks, const uint8_t *data, uint64_t len,
                     uint8_t *tags, uint32_t flags, uint64_t *tries_out);

/* hb_encode_many for the cxx Swizzle (heartbeat.Heartbeat): many whole files,
 * each under its own keys, in one call.
 * Replaces a caller's loop over cxx/shacham_waters_private.cxx:638-702 with
 * the prf of cxx/prf.hxx:125-176: file i's tags are exactly the bytes that
 * hb_encode writes for it with HB_PRF_CXX, block_base = 0 and nblocks =
 * hb_block_count(p, sectors, len) -- a block that reads no sector (the last
 * one of a file whose length is a multiple of the block size; the only one of
 * an empty file) keeps F as the prf returned it (:681-690).  Same descriptors
 * as hb_encode_many; one prime, one `sectors` and one key_len for the batch.
 * A try of the cxx prf is ByteCount(p) / 16 full AES blocks, so the single
 * call is bound by its launches, not by a chain: here a group of files is one
 * PRF launch (one lane per evaluation, wave-jobs of up to 64 evaluations of
 * one file under one key, longest first), one Montgomery pass over the
 * group's alpha values and one MAC launch, with one copy up and one down.
 * Files with more blocks than hb_encode_many batches go through
 * hb_encode(HB_PRF_CXX) inside the same call, so any mix of sizes is accepted.
 * Every file is checked before any GPU work and hb_last_error names the
 * rejected file's index ("file 3: ..."); what hb_encode(HB_PRF_CXX) rejects
 * fails the whole call with that call's code -- a prime whose ByteCount is not
 * a multiple of 16 with HB_EUNSUPPORTED -- and no tag buffer is written.
 * flags: HB_DATA_ON_DEVICE and/or HB_TAGS_ON_DEVICE (device pointers of any
 * alignment); anything else returns HB_EUNSUPPORTED.  nfiles == 0 returns
 * HB_OK.  *tries_out (may be NULL) receives the sum of the files' F tries:
 * what nfiles hb_encode calls report in total. */
int hb_cxx_encode_many(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
                       size_t key_len, const hb_file_desc *files, uint64_t nfiles,
                       uint32_t flags, uint64_t *tries_out);

/* hb_encode_blocks_many for the cxx Swizzle (heartbeat.Heartbeat): the tags of
 * listed blocks -- those an edit or an append changed -- of one file or of
 * many files each under its own keys, in one call, under the file's existing
 * keys.  Same descriptors as hb_encode_blocks_many (hb_blocks_desc).
 * Replaces a caller's loop over the body of cxx/shacham_waters_private.cxx:674-694
 * for chosen values of i: tags[k] of a file are exactly the bytes that
 * hb_encode writes with HB_PRF_CXX for block_base = indices[k], data + k*C,
 * len_k = min(C, len - k*C) and nblocks = 1, with C = sectors * ss.  Only the
 * last listed block may be short; when it is empty it reads no sector and its
 * tag is F(indices[k]) as the prf returned it, without `%= p` (:681-690).
 * indices may come in any order and may repeat.  One prime, one `sectors` and
 * one key_len for the batch.  A group of lists is one copy up (key schedules,
 * u32 indices and host data together), one PRF launch (one lane per
 * evaluation, wave-jobs of up to 64 evaluations of one list under one key: F
 * at the listed indices and alpha_j of every file), one Montgomery pass over
 * the group's alpha values, hb_encode_many's MAC launch over the packed blocks
 * that read a sector, and one copy down; the runtime splits a call, and a
 * single list, whose device scratch would pass the batches' cap
 * ($HB_TEST_BATCH_BLOCKS: at that many listed blocks), and nothing goes
 * through the single encode.
 * Everything is checked before any GPU work, no tag buffer is written on a
 * failure, and the checks run in this order:
 *   1. the context, the prime, key_len (16, 24 or 32), sectors > 0;
 *   2. flags: anything but HB_DATA_ON_DEVICE / HB_TAGS_ON_DEVICE (device
 *      pointers of any alignment) returns HB_EUNSUPPORTED;
 *   3. nfiles == 0 returns HB_OK; then files == NULL is HB_EINVAL;
 *   4. every descriptor as hb_encode_blocks_many checks it -- per file keys,
 *      indices, len, tags, data; the first fault of the first faulty file --
 *      with HB_EINVAL and "file N: ...";
 *   5. every index, file by file: one of 2^32 or above returns
 *      HB_EUNSUPPORTED with "file N: index ..." (the reference's chunk_id is
 *      an unsigned int and the cxx prove refuses 2^32 tags; a wrapped index
 *      would collide silently);
 *   6. a prime whose ByteCount is not a multiple of 16: HB_EUNSUPPORTED, as
 *      hb_encode(HB_PRF_CXX).
 * A file with nblocks == 0 is a no-op.  *tries_out (may be NULL) receives the
 * sum of the listed blocks' F tries: what those single hb_encode calls report
 * in total. */
int hb_cxx_encode_blocks_many(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
                              size_t key_len, const hb_blocks_desc *files, uint64_t nfiles,
                              uint32_t flags, uint64_t *tries_out);

/* hb_cxx_encode_blocks_many for one file (nfiles = 1; errors read "file 0: ..."). */
int hb_cxx_encode_blocks(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
                         const uint8_t *f_key, const uint8_t *alpha_key, size_t key_len,
                         const uint64_t *indices, uint64_t nblocks, const uint8_t *data, uint64_t len,
                         uint8_t *tags, uint32_t flags, uint64_t *tries_out);

/* The cxx prf, prf::evaluate(i) (cxx/prf.hxx:125-145), for n unsigned-int
 * inputs, keyed by key and bounded by limit (any limit up to 2048 bits; when
 * ByteCount(limit) is not a multiple of 16 the CFB-128 stream continues
 * mid-block across tries): out receives n values of ByteCount(limit)
 * big-endian bytes each. */
int hb_cxx_prf_eval(hb_ctx *ctx, const uint8_t *key, size_t key_len,
                    const uint8_t *limit_be, size_t limit_len,
                    const uint32_t *xs, size_t n, uint8_t *out);

/* len/C + 1: the number of tags PySwizzle.encode produces for a file. */
uint64_t hb_block_count(const uint8_t *p_be, size_t p_len, uint32_t sectors,
                        uint64_t len);

/* Swizzle prove.
 * Replaces heartbeat/PySwizzle/PySwizzle.py:333-370 and
 * cxx/shacham_waters_private.cxx:731-789:
 *   idx_i = KeyedPRF(chal_key, ntags)(i), v_i = KeyedPRF(chal_key, v_max)(i)
 *   mu_j  = sum_i v_i * m_{idx_i, j} mod p      (i < chunks)
 *   sigma = sum_i v_i * tags[idx_i]    mod p
 * tags: ntags * hb_width(p) bytes.  data: the whole file (len bytes).
 * mu_out: sectors * hb_width(p) bytes, sigma_out: hb_width(p) bytes (host).
 * With HB_PRF_CXX: the cxx extension's prove (shacham_waters_private.cxx:731-789)
 * -- idx_i and v_i from the cxx prf (cxx/prf.hxx), every block in order when
 * chunks >= ntags (check_all, :754-762), and block offsets computed as
 * (unsigned int)(idx * sectors * ss) like the reference (:738, 763; differs
 * from PySwizzle for blocks past 4 GiB).  Parity unpinned (Crypto++ absent). */
int hb_prove(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
             const uint8_t *chal_key, size_t key_len, uint64_t chunks,
             const uint8_t *vmax_be, size_t vmax_len,
             const uint8_t *tags, uint64_t ntags,
             const uint8_t *data, uint64_t len, uint32_t flags,
             uint8_t *mu_out, uint8_t *sigma_out);

/* The part of hb_prove over challenge indices [chunk_begin, chunk_end) of a
 * `chunks`-index challenge: mu_out / sigma_out receive that range's sums mod p.
 * The sums of a partition of [0, chunks) add (mod p) to hb_prove's result:
 * a prove sharded over several GPUs (one context each) is one call per GPU
 * plus a host-side sum of S + 1 values mod p.  hb_prove is chunk_begin = 0,
 * chunk_end = UINT64_MAX.  Replaces the same loop as hb_prove
 * (PySwizzle.py:351-368; cxx shacham_waters_private.cxx:757-788). */
int hb_prove_range(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
                   const uint8_t *chal_key, size_t key_len, uint64_t chunks,
                   uint64_t chunk_begin, uint64_t chunk_end,
                   const uint8_t *vmax_be, size_t vmax_len,
                   const uint8_t *tags, uint64_t ntags,
                   const uint8_t *data, uint64_t len, uint32_t flags,
                   uint8_t *mu_out, uint8_t *sigma_out);

/* mu and sigma of many proofs, each under its own challenge key, file and tag
 * array, in one call.  Replaces a storage node's loop of hb_prove over the
 * challenges of an audit period (PySwizzle.py:333-370 per proof): proof i's
 * mu_out and sigma_out receive exactly the bytes hb_prove writes for the same
 * arguments, PySwizzle's KeyedPRF.  One prime, one `sectors` and one key_len
 * (16, 24 or 32) for the batch; everything else per proof.  A single prove of
 * a small file is bound by the latency of its longest PRF rejection chain on
 * a few dozen waves; the batch runs the chains of all proofs side by side --
 * per group of proofs one H2D copy, one PRF launch, a Montgomery pass over
 * the group's v, one sum launch and one D2H copy (the runtime splits a batch
 * whose device scratch, uploaded files included, would pass its cap).
 * flags applies to the whole batch: HB_DATA_ON_DEVICE and/or
 * HB_TAGS_ON_DEVICE (device pointers of any alignment); anything else
 * (HB_PRF_CXX, HB_ASYNC, ...) returns HB_EUNSUPPORTED.  A host-resident file
 * is batched when hb_prove would upload it whole (len <= max(2 chunks C,
 * 8 MiB), C = sectors * sector size); its bytes and host tags go up in the
 * group's one copy.  Proofs that path does not take (more challenge indices
 * than the quad engine places, a larger host file, host data with device
 * tags) go through the single prove inside the same call, so any mix is
 * accepted and the results are the same.  chunks == 0 gives zero mu and
 * sigma.  nproofs == 0 returns HB_OK.  A descriptor that hb_prove would
 * reject (ntags == 0, v_max == 0, a v_max wider than the prime's limb count
 * -- also with chunks == 0) fails the whole call with the code hb_prove
 * returns, before any GPU work, and so does a NULL key, result buffer, tags,
 * or data with len > 0 (HB_EINVAL); hb_last_error names the proof's index. */
typedef struct hb_prove_desc {        /* ten 8-byte words, in this order */
    const uint8_t *chal_key;          /* key_len bytes */
    uint64_t chunks;
    const uint8_t *vmax_be;
    uint64_t vmax_len;
    const uint8_t *tags;              /* ntags * hb_width(p) bytes; host, or device with HB_TAGS_ON_DEVICE */
    uint64_t ntags;
    const uint8_t *data;              /* the whole file; host, or device with HB_DATA_ON_DEVICE; may be NULL when len == 0 */
    uint64_t len;
    uint8_t *mu_out;                  /* sectors * hb_width(p) bytes, host */
    uint8_t *sigma_out;               /* hb_width(p) bytes, host */
} hb_prove_desc;

int hb_prove_many(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
                  size_t key_len, const hb_prove_desc *proofs, uint64_t nproofs, uint32_t flags);

/* Right-hand side of PySwizzle.verify (PySwizzle.py:381-394) for a decrypted
 * state:  rhs = sum_i v_i * F(idx_i) + sum_j alpha(j) * mu_j  mod p.
 * The caller compares rhs with proof.sigma.  mu: sectors * hb_width(p) bytes
 * (each value must be < 2^(8*width)). */
int hb_verify_rhs(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
                  const uint8_t *f_key, const uint8_t *alpha_key, size_t key_len,
                  uint64_t state_chunks,
                  const uint8_t *chal_key, size_t chal_key_len, uint64_t chunks,
                  const uint8_t *vmax_be, size_t vmax_len,
                  const uint8_t *mu, uint8_t *rhs_out);

/* The right-hand sides of many proofs, each under its own keys, in one call.
 * Replaces an auditor's loop of hb_verify_rhs over the proofs that came back
 * for its challenges (PySwizzle.py:381-394 per proof): proof i's rhs_out
 * receives exactly the bytes hb_verify_rhs writes for the same arguments,
 * PySwizzle's KeyedPRF.  One prime, one `sectors`, one key_len and one
 * chal_key_len (16, 24 or 32 each) for the batch; the state's keys and chunk
 * count, the challenge's key, chunk count and v_max, mu and the result buffer
 * per proof; all buffers are host memory.  A single verify is bound by the
 * latency of its longest PRF rejection chain on a few dozen waves; the batch
 * runs the chains of all proofs side by side -- one PRF launch and one sum
 * launch per group of proofs (the runtime splits a batch whose device scratch
 * would pass its cap) -- and proofs that path does not take (more challenge
 * indices than the quad engine places, or key_len and chal_key_len with
 * different AES round counts) go through the single verify inside the same
 * call, so any mix is accepted and the results are the same.
 * flags must be 0 (anything else returns HB_EUNSUPPORTED).  nproofs == 0
 * returns HB_OK.  A descriptor that hb_verify_rhs would reject (state_chunks
 * == 0 with chunks > 0, v_max == 0 with chunks > 0, a v_max wider than the
 * prime's limb count, a NULL buffer) fails the whole call with the code
 * hb_verify_rhs returns, before any GPU work, and hb_last_error names the
 * proof's index.  The mu values go up and the results come back in one copy
 * each per group. */
typedef struct hb_verify_desc {        /* nine 8-byte words, in this order */
    const uint8_t *f_key, *alpha_key;  /* key_len bytes each (decrypted state) */
    const uint8_t *chal_key;           /* chal_key_len bytes */
    uint64_t state_chunks, chunks;
    const uint8_t *vmax_be;            /* may be NULL when chunks == 0 */
    uint64_t vmax_len;
    const uint8_t *mu;                 /* sectors * hb_width(p) bytes */
    uint8_t *rhs_out;                  /* hb_width(p) bytes */
} hb_verify_desc;

int hb_verify_rhs_many(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
                       size_t key_len, size_t chal_key_len,
                       const hb_verify_desc *proofs, uint64_t nproofs, uint32_t flags);

/* hb_prove_many for the proofs of many owners: every proof names its own
 * prime, `sectors` and challenge key length.  A PySwizzle instance draws its
 * own prime (PySwizzle.py:250-251) and hands it to the storage node with the
 * public beat (:277), so a node that answers an audit period's challenges for
 * several owners has one prime per owner, not one per batch.  Replaces that
 * node's loop of hb_prove (PySwizzle.py:333-370 per proof): proof i's mu_out
 * (its own sectors * hb_width(its own p) bytes) and sigma_out receive exactly
 * the bytes hb_prove writes for the same arguments, PySwizzle's KeyedPRF.
 * The proofs are split into classes by the prime's limb count (256 / 512 /
 * 1024 / 2048 bits) and the key's AES round count; a class is grouped and run
 * as hb_prove_many runs a batch -- per group one H2D copy, one PRF launch,
 * one conversion pass, one sum launch, one D2H copy -- with each proof's
 * modulus, geometry and result columns in a per-proof device record.  The
 * Montgomery constants are computed once per distinct prime of the call.
 * Proofs the batch path does not take (as in hb_prove_many: more challenge
 * indices than the quad engine places, a host file above max(2 chunks C,
 * 8 MiB), host data with device tags) go through the single prove under their
 * own prime and `sectors` inside the same call.
 * flags applies to the whole call: HB_DATA_ON_DEVICE and/or
 * HB_TAGS_ON_DEVICE; anything else returns HB_EUNSUPPORTED.  nproofs == 0
 * returns HB_OK; chunks == 0 gives zero mu and sigma.  Every descriptor is
 * checked before any GPU work: what hb_prove rejects for that proof's own
 * arguments (a prime above 2048 bits or below 2^7, an even prime, sectors ==
 * 0, a key length other than 16 / 24 / 32, ntags == 0, v_max == 0, a v_max
 * wider than THAT proof's limb count, a NULL buffer) fails the whole call
 * with hb_prove's code, hb_last_error names the proof ("proof 3: ..."), and
 * no result buffer is written. */
typedef struct hb_prove_mixed_desc {  /* fourteen 8-byte words, in this order */
    const uint8_t *p_be;              /* this proof's prime, big-endian */
    uint64_t p_len;
    uint64_t sectors;                 /* this proof's S (below 2^32) */
    uint64_t key_len;                 /* chal_key bytes: 16, 24 or 32 */
    hb_prove_desc d;                  /* the ten words of hb_prove_desc, same meaning */
} hb_prove_mixed_desc;

int hb_prove_mixed(hb_ctx *ctx, const hb_prove_mixed_desc *proofs, uint64_t nproofs, uint32_t flags);

/* hb_verify_rhs_many for the proofs of many owners: every proof names its own
 * prime, `sectors`, state key length and challenge key length.  Replaces an
 * auditor's loop of hb_verify_rhs over the proofs of several owners
 * (PySwizzle.py:381-394 per proof): proof i's rhs_out (hb_width(its own p)
 * bytes) receives exactly the bytes hb_verify_rhs writes for the same
 * arguments.  Classes (limb count, AES round count), groups and launches
 * (one PRF launch, one sum launch per group) as in hb_prove_mixed; a proof
 * whose key_len and chal_key_len have different round counts, or with more
 * challenge indices than the quad engine places, goes through the single
 * verify under its own prime inside the same call.  flags must be 0 (anything
 * else returns HB_EUNSUPPORTED); nproofs == 0 returns HB_OK.  Every
 * descriptor is checked before any GPU work with hb_verify_rhs's rules and
 * codes for that proof's own arguments; hb_last_error names the proof and no
 * result buffer is written. */
typedef struct hb_verify_mixed_desc { /* fourteen 8-byte words, in this order */
    const uint8_t *p_be;
    uint64_t p_len;
    uint64_t sectors;
    uint64_t key_len, chal_key_len;   /* f_key / alpha_key bytes; chal_key bytes */
    hb_verify_desc d;                 /* the nine words of hb_verify_desc, same meaning */
} hb_verify_mixed_desc;

int hb_verify_rhs_mixed(hb_ctx *ctx, const hb_verify_mixed_desc *proofs, uint64_t nproofs, uint32_t flags);

/* Right-hand side of the cxx extension's verify (shacham_waters_private.cxx:
 * 791-842) for a decrypted state: the same sum as hb_verify_rhs with the cxx
 * prf (cxx/prf.hxx) for index, v, f and alpha, and every block in order when
 * chunks >= state_chunks (check_all, :822-827).  Parity unpinned. */
int hb_cxx_verify_rhs(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
                      const uint8_t *f_key, const uint8_t *alpha_key, size_t key_len,
                      uint64_t state_chunks,
                      const uint8_t *chal_key, size_t chal_key_len, uint64_t chunks,
                      const uint8_t *vmax_be, size_t vmax_len,
                      const uint8_t *mu, uint8_t *rhs_out);

/* hb_prove_many for the cxx Swizzle (heartbeat.Heartbeat): mu and sigma of
 * many proofs, each under its own challenge key, file and tag array, in one
 * call.  Replaces a storage node's loop over
 * cxx/shacham_waters_private.cxx:731-789 with the prf of cxx/prf.hxx:125-176:
 * proof i's mu_out and sigma_out receive exactly the bytes that hb_prove
 * writes for the same arguments with flags | HB_PRF_CXX.  Same descriptors as
 * hb_prove_many; one prime, one `sectors` and one key_len for the batch.
 * The cxx semantics are the single call's: every block in order, without the
 * index prf, when chunks >= ntags (check_all, :754-762; the default Swizzle
 * audit); otherwise idx_i from the byte-granular prf on the limit ntags with
 * the 81-try forced accept (prf.hxx:135-142); sector offsets in unsigned int
 * (:738, 762-763).  An index that the forced accept leaves >= ntags (below
 * 2^-81 per index) contributes zero and fails the call with HB_EINVAL
 * "proof i: vector::_M_range_check..." as the single call does; no address is
 * formed from it.  A try of the cxx prf is ByteCount(limit) / 16 full AES
 * blocks, so the single call is bound by its launches and synchronisations:
 * here a group of proofs is one copy up, one PRF launch (one lane per
 * evaluation, wave-jobs of up to 64 evaluations of one proof under one key),
 * one Montgomery pass over the group's v, one sum launch (a workgroup per
 * proof and column) and one copy down.  Through hb_prove(HB_PRF_CXX) inside
 * the same call, with identical results: every proof when ByteCount(p) is not
 * a multiple of 16; a proof whose ByteCount(v_max) is not, with host data and
 * device tags, with a host file above max(2 n C, 8 MiB) (n the effective chunk
 * count, C = sectors * sector size), or that alone passes the group's scratch
 * cap.  A batched host file and its host tags go up in the group's one copy.
 * Every descriptor is checked before any GPU work, with hb_prove_many's rules
 * and codes, and hb_last_error names the proof's index; ntags >= 2^32 returns
 * HB_EUNSUPPORTED.  chunks == 0 gives zero mu and sigma.  nproofs == 0 returns
 * HB_OK.  flags: HB_DATA_ON_DEVICE and/or HB_TAGS_ON_DEVICE; anything else
 * returns HB_EUNSUPPORTED.  Parity unpinned (Crypto++ absent). */
int hb_cxx_prove_many(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
                      size_t key_len, const hb_prove_desc *proofs, uint64_t nproofs, uint32_t flags);

/* hb_verify_rhs_many for the cxx Swizzle: the right-hand sides of many
 * proofs, each under its own keys, in one call.  Replaces an auditor's loop
 * over cxx/shacham_waters_private.cxx:791-842 with the prf of
 * cxx/prf.hxx:125-176: proof i's rhs_out receives exactly the bytes that
 * hb_cxx_verify_rhs writes for the same arguments.  Same descriptors as
 * hb_verify_rhs_many.  check_all when chunks >= state_chunks (:822-827): F(i)
 * of every block in order, v_i = prf(chal_key, v_max)(i), no index prf;
 * otherwise the lane that evaluates F draws idx_i first (byte-granular prf on
 * the limit state_chunks, forced accept after 81 tries) and F takes any index
 * (verify has no range check).  A group of proofs is one copy up, one PRF
 * launch (v, F and alpha of every proof), one sum launch (a workgroup per
 * proof) and one copy down.  Through hb_cxx_verify_rhs inside the same call,
 * with identical results: every proof when ByteCount(p) is not a multiple of
 * 16 or key_len and chal_key_len have different AES round counts; a proof
 * whose ByteCount(v_max) is not a multiple of 16 or that alone passes the
 * group's scratch cap.  Every descriptor is checked before any GPU work, with
 * hb_verify_rhs_many's rules and codes (state_chunks >= 2^32:
 * HB_EUNSUPPORTED, as hb_cxx_verify_rhs), and hb_last_error names the proof's
 * index.  chunks == 0 gives sum_j alpha_j mu_j.  nproofs == 0 returns HB_OK.
 * flags must be 0.  Parity unpinned. */
int hb_cxx_verify_rhs_many(hb_ctx *ctx, const uint8_t *p_be, size_t p_len, uint32_t sectors,
                           size_t key_len, size_t chal_key_len,
                           const hb_verify_desc *proofs, uint64_t nproofs, uint32_t flags);

/* hb_cxx_prove_many for the proofs of many owners: every proof names its own
 * prime, `sectors` and challenge key length.  Every cxx Swizzle draws its own
 * prime (init, cxx/shacham_waters_private.cxx:596-624) and hands it to the
 * storage node with the public beat, so a node that answers an audit period's
 * challenges for several owners has one prime per owner.  Replaces that node's
 * loop over cxx/shacham_waters_private.cxx:731-789 with the prf of
 * cxx/prf.hxx:125-176 (one hb_prove with HB_PRF_CXX per proof): proof i's
 * mu_out (its own sectors * hb_width(its own p) bytes) and sigma_out receive
 * exactly the bytes hb_prove(..., flags | HB_PRF_CXX, ...) writes for that
 * proof's own arguments, check_all when chunks >= ntags and the (unsigned
 * int) sector offsets under that proof's own sectors * sector size included.
 * Takes hb_prove_mixed_desc unchanged.  Classes (limb count, AES round count)
 * as in hb_prove_mixed; a class is grouped and run as hb_cxx_prove_many runs a
 * batch -- per group one H2D copy, one PRF launch, one conversion pass, one
 * sum launch, one D2H copy -- with each proof's modulus, geometry and result
 * columns in a per-proof device record; Montgomery constants once per
 * distinct prime.  A proof goes through the single cxx prove under its own
 * prime and `sectors` inside the same call, with identical results, when
 * ByteCount(its p) or ByteCount(its v_max) is not a multiple of 16, with host
 * data and device tags, with a host file above max(2 n C, 8 MiB) (n: its
 * effective chunks, C: its own), or when it alone exceeds the runtime's
 * scratch cap.  flags: HB_DATA_ON_DEVICE and/or HB_TAGS_ON_DEVICE; anything
 * else returns HB_EUNSUPPORTED.  nproofs == 0 returns HB_OK; a proof with
 * chunks == 0 gets zero mu and sigma and no GPU work.  Every descriptor is
 * checked before any GPU work with hb_prove(HB_PRF_CXX)'s rules and codes for
 * that proof's own prime, sectors, key length and arguments (ntags >= 2^32:
 * HB_EUNSUPPORTED); hb_last_error names the proof ("proof 3: ...") and no
 * result buffer is written.  Parity unpinned, as every cxx entry point. */
int hb_cxx_prove_mixed(hb_ctx *ctx, const hb_prove_mixed_desc *proofs, uint64_t nproofs, uint32_t flags);

/* hb_cxx_verify_rhs_many for the proofs of many owners: every proof names its
 * own prime, `sectors`, state key length and challenge key length.  Replaces
 * an auditor's loop over cxx/shacham_waters_private.cxx:791-842 with the prf
 * of cxx/prf.hxx:125-176 (one hb_cxx_verify_rhs per proof): proof i's rhs_out
 * (hb_width(its own p) bytes) receives exactly the bytes hb_cxx_verify_rhs
 * writes for the same arguments.  Takes hb_verify_mixed_desc unchanged.
 * Classes, groups and launches (one PRF launch, one sum launch per group) as
 * in hb_cxx_prove_mixed; a proof whose key_len and chal_key_len have different
 * AES round counts, whose prime's or v_max's ByteCount is not a multiple of
 * 16, or which alone exceeds the scratch cap goes through hb_cxx_verify_rhs's
 * path under its own prime inside the same call.  flags must be 0 (anything
 * else returns HB_EUNSUPPORTED); nproofs == 0 returns HB_OK.  Every
 * descriptor is checked before any GPU work with hb_cxx_verify_rhs's rules
 * and codes for that proof's own arguments (state_chunks >= 2^32:
 * HB_EUNSUPPORTED); hb_last_error names the proof and no result buffer is
 * written. */
int hb_cxx_verify_rhs_mixed(hb_ctx *ctx, const hb_verify_mixed_desc *proofs, uint64_t nproofs, uint32_t flags);

/* hb_encode_many for the files of many owners: every file names its own
 * prime, `sectors` and key length.  A PySwizzle instance draws its own prime
 * (heartbeat/PySwizzle/PySwizzle.py:250-251), so a process that keeps one beat
 * per owner, contract or farmer and tags one file for each has one prime per
 * file, not one per batch.  Replaces that process's loop of hb_encode
 * (PySwizzle.py:279-311 per file): file i's tag buffer
 * (hb_block_count(its own p, its own sectors, len) * hb_width(its own p)
 * bytes) receives exactly the bytes hb_encode writes for the same prime,
 * sectors, keys and data with block_base = 0 and nblocks = hb_block_count(...),
 * PySwizzle's KeyedPRF.  The files are split into classes by the prime's limb
 * count (256 / 512 / 1024 / 2048 bits) and the key's AES round count; a class
 * is grouped under hb_encode_many's caps and a group is one H2D copy, three
 * launches -- the PRF launch (F of every block, alpha of every sector, each
 * file's schedules with its own range), a conversion pass alpha -> alpha R
 * mod p over the group's alpha slots under each file's modulus, and one MAC
 * launch whose workgroups each take blocks of one file and read that file's
 * modulus, block size, sector size, sector count, tag width and first alpha
 * slot from a per-file device record -- and one D2H copy.  The Montgomery
 * constants are computed once per distinct prime of the call.  A file with
 * more blocks than hb_encode_many batches, or which alone exceeds the group's
 * scratch cap, goes through the single encode under its own prime and
 * `sectors` inside the same call.
 * flags applies to the whole call and means what it means in hb_encode_many:
 * HB_DATA_ON_DEVICE / HB_TAGS_ON_DEVICE (device pointers of any alignment);
 * HB_HOST_REGISTER is ignored; HB_PRF_CXX, HB_ASYNC and HB_ENCODE_SINGLE_PASS
 * return HB_EUNSUPPORTED.  nfiles == 0 returns HB_OK.  Every descriptor is
 * checked before any GPU work with hb_encode's rules and codes for that
 * file's own arguments (a prime above 2048 bits or below 2^8, an even prime,
 * sectors == 0 or not below 2^32, a key length other than 16 / 24 / 32, a NULL
 * key or tag buffer, a NULL data buffer with len > 0); hb_last_error names the
 * file ("file 3: ...") and no tag buffer is written.  *tries_out (may be
 * NULL) receives the sum of the files' F tries: what nfiles hb_encode calls
 * report in total. */
typedef struct hb_encode_mixed_desc {  /* nine 8-byte words, in this order */
    const uint8_t *p_be;               /* this file's prime, big-endian */
    uint64_t p_len;
    uint64_t sectors;                  /* this file's S (below 2^32) */
    uint64_t key_len;                  /* f_key / alpha_key bytes: 16, 24 or 32 */
    hb_file_desc d;                    /* the five words of hb_file_desc, same meaning */
} hb_encode_mixed_desc;

int hb_encode_mixed(hb_ctx *ctx, const hb_encode_mixed_desc *files, uint64_t nfiles,
                    uint32_t flags, uint64_t *tries_out);

/* hb_cxx_encode_many for the files of many owners: every cxx Swizzle draws
 * its own prime (init, cxx/shacham_waters_private.cxx:596-624).  Replaces a
 * loop over cxx/shacham_waters_private.cxx:638-702 with the prf of
 * cxx/prf.hxx:125-176 (one hb_encode with HB_PRF_CXX per file): file i's tags
 * are exactly the bytes hb_encode(..., HB_PRF_CXX) writes for that file's own
 * prime, sectors, keys and data with block_base = 0 and nblocks =
 * hb_block_count(...); a block that reads no sector under the file's OWN
 * block size (the last one of a file whose length is a multiple of it; the
 * only one of an empty file) keeps F as the prf returned it (:681-690).
 * Takes hb_encode_mixed_desc unchanged.  Classes, groups and fall-through as
 * in hb_encode_mixed; a group is one H2D copy, the PRF launch (one lane per
 * evaluation, wave-jobs of up to 64 evaluations of one file under one key,
 * longest first), the conversion pass, the MAC launch of hb_encode_mixed
 * (none when no block of the group reads a sector) and one D2H copy.
 * flags: HB_DATA_ON_DEVICE and/or HB_TAGS_ON_DEVICE; anything else returns
 * HB_EUNSUPPORTED.  nfiles == 0 returns HB_OK.  Every descriptor is checked
 * before any GPU work with hb_encode(HB_PRF_CXX)'s rules and codes for that
 * file's own arguments -- a prime whose ByteCount is not a multiple of 16
 * fails the call with HB_EUNSUPPORTED -- hb_last_error names the file and no
 * tag buffer is written.  Parity unpinned, as every cxx entry point. */
int hb_cxx_encode_mixed(hb_ctx *ctx, const hb_encode_mixed_desc *files, uint64_t nfiles,
                        uint32_t flags, uint64_t *tries_out);

/* Strong-probable-prime tests, a lane per (candidate, base).  Replaces the
 * Miller-Rabin rounds of getPrime (PySwizzle.py:74-77): many candidates and
 * many bases in one launch, each lane deriving its own Montgomery constants
 * (csrc/hb_prime.hpp).  Deterministic: the bases come from the caller.
 *
 * cands_be: ncands numbers of `width` bytes each (1..256, big-endian, leading
 * zero bytes allowed), every one odd and >= 5; the limb class is the smallest
 * that holds `width`.  bases_be: ncands x rounds x width bytes, base r of
 * candidate i at (i * rounds + r) * width, each in [2, n_i - 2]; 1 <= rounds
 * <= 65536.  verdicts[i] = 1 iff candidate i is a strong probable prime to
 * EACH of its bases, else 0.  That is the exact function, not "is prime":
 * 3215031751 = 151 * 751 * 28351 with bases 2, 3, 5, 7 gives 1.
 * ncands == 0: HB_OK.  A bad argument (an even candidate, one below 5, a base
 * outside [2, n - 2], rounds == 0): HB_EINVAL, hb_last_error names the
 * candidate, and no verdict is written.  width > 256 (or > 128 in a build
 * without the 2048-bit kernels), rounds > 65536: HB_EUNSUPPORTED.
 * hb_last_kernel_ms's launch count covers this call. */
int hb_mr_test(hb_ctx *ctx, const uint8_t *cands_be, size_t width, uint64_t ncands,
               const uint8_t *bases_be, uint32_t rounds, uint8_t *verdicts);

/* Incremental prime search from many starts at once.  Replaces a loop of
 * getPrime (PySwizzle.py:74-77, one prime per owner object, :250-251).
 *
 * 8 <= bits <= 2048, width = ceil(bits / 8), 1 <= window <= 65536, rounds <=
 * 65536 (0: base 2 alone; bases_be may then be NULL).  starts_be: nstarts x
 * width bytes, each start odd with exactly `bits` bits.  bases_be: nstarts x
 * rounds x width bytes, each base in [2, 2^(bits-1) - 1], which is inside
 * [2, n - 2] for every candidate of that size.
 * The result for start i is the SMALLEST n = start_i + 2k, 0 <= k < window,
 * n < 2^bits, that is a strong probable prime to base 2 and to every
 * bases_i[r]: found[i] = 1 and n in primes_be[i * width ..], big-endian; if
 * there is none, found[i] = 0 and that slot is zero bytes.  How it gets there
 * does not change that definition: a sieve by the odd primes below 2^16 per
 * start (a candidate that is itself such a prime survives), base 2 tests over
 * batches of survivors in ascending order, then a lane per base for the
 * earliest survivor that passed; no candidate is reported unless every
 * smaller survivor was tested and failed (csrc/hb_prime_host.hpp).
 * *tests_out (may be NULL): the number of lane tests run.  nstarts == 0:
 * HB_OK.  A bad argument: HB_EINVAL, hb_last_error names the start, nothing
 * is written. */
int hb_prime_search(hb_ctx *ctx, uint32_t bits, const uint8_t *starts_be, uint64_t nstarts,
                    uint32_t window, const uint8_t *bases_be, uint32_t rounds,
                    uint8_t *primes_be, uint8_t *found, uint64_t *tests_out);

/* Host AES-CFB8(segment 8, any 16-byte IV) for PySwizzle State
 * encrypt/decrypt (PySwizzle.py:162-195): 64 bytes per call, not a hot path.
 * encrypt = 1 encrypts, 0 decrypts. */
int hb_aes_cfb8(const uint8_t *key, size_t key_len, const uint8_t *iv,
                const uint8_t *in, uint8_t *out, size_t n, int encrypt);

/* Host AES-CFB128 (full-block feedback, no padding) for the cxx extension's
 * State encrypt-and-sign (cxx/shacham_waters_private.cxx:169-306, Crypto++
 * CFB_Mode<AES>): a few dozen bytes per call, not a hot path. */
int hb_aes_cfb128(const uint8_t *key, size_t key_len, const uint8_t *iv,
                  const uint8_t *in, uint8_t *out, size_t n, int encrypt);

/* Device timing of the last hb_encode on this context: milliseconds spent in
 * the encode kernel (HIP events on the kernel's stream), and launch count.  A
 * pending HB_ASYNC encode is completed first (its status stays for
 * hb_ctx_wait). */
int hb_last_kernel_ms(hb_ctx *ctx, double *ms, uint32_t *launches);

/* Phase times of the last device-resident two-pass encode on this context
 * (ms[0..3]: the set-up kernels -- prefix image, MAC tables --, the first-try
 * pass, the retry pass, the split wide-prime MAC (0 when the MAC ran inside the
 * PRF passes)), from events between its launches.  Returns the number of
 * values written (at most n and 4; 0 when the last encode was not such a
 * launch), negative on error.  Replaces nothing in the reference
 * (instrumentation, like hb_last_kernel_ms). */
int hb_last_kernel_phases(hb_ctx *ctx, double *ms, uint32_t n);

/* Device memory helpers so that callers without a GPU framework (e.g. a cgo or
 * JNI binding) can hold a device-resident file: allocate, copy
 * (kind 1 = host->device, 2 = device->host, 3 = device->device), free. */
int hb_device_malloc(hb_ctx *ctx, uint64_t bytes, void **out);
int hb_device_free(hb_ctx *ctx, void *ptr);
int hb_memcpy(hb_ctx *ctx, void *dst, const void *src, uint64_t bytes, int kind);

/* Page-lock (pin) an existing host buffer for the device of ctx, e.g. the file
 * bytes and the tag buffer of a host-path hb_encode: pinned chunks are copied
 * by DMA at the full PCIe rate and overlap the encode of the previous chunk
 * (pageable ones go through a driver staging copy).  The reference reads the
 * file through Python read() calls (PySwizzle.py:299; cxx/PythonSeekableFile.hxx:47-54);
 * this is the native replacement's staging.  Unregister before freeing. */
int hb_host_register(hb_ctx *ctx, void *ptr, uint64_t bytes);
int hb_host_unregister(hb_ctx *ctx, void *ptr);

/* Fill len bytes of device memory with the synthetic SplitMix64 stream used by
 * the benchmarks and tests: byte k = byte (k mod 8) (little-endian) of
 * splitmix64(seed ^ (2*(k/16) + ((k mod 16) >= 8)) * 0xD1B54A32D192ED03). */
int hb_fill_random(hb_ctx *ctx, uint8_t *dev_ptr, uint64_t len, uint64_t seed);

/* Measurement helper (no reference counterpart): read len bytes of device
 * memory once with streaming 16-byte loads; *ms = kernel time.  bench.py
 * reports len / ms as the measured HBM read peak beside the vendor figure. */
int hb_stream_read(hb_ctx *ctx, const void *dev_ptr, uint64_t len, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* HBSWIZZLE_H */
