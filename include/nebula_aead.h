/*
 * nebula_aead.h — C ABI of the MI355X (gfx950) AEAD engine for Nebula's per-packet data plane.
 *
 * Plain C: pointers, sizes and integers only; no torch or HIP types cross this boundary
 * (streams are passed as `void*` = hipStream_t). Every entry point returns an int status
 * (NEB_OK = 0, negative = error); nothing throws across the ABI.
 *
 * Reference interfaces replaced (slackhq/nebula, /root/reference):
 *   neb_cipher_create        noise.CipherFunc.Cipher(k [32]byte) — flynn/noise v1.1.0 [ext]; the
 *                            reference's own CipherFunc pattern is noiseutil/fips140.go:31-40,
 *                            selected at pki.go:263-269; wrapped by noiseutil.NewCipherState
 *                            (noiseutil/cipher_state.go:42-54, plugin hook :43-45)
 *   neb_cipher_name          noise.CipherFunc.CipherName() ("AESGCM" / "ChaChaPoly")
 *   neb_encrypt_danger       CipherState.EncryptDanger  noiseutil/cipher_state.go:32,
 *                            noiseutil/aesgcm.go:24-37, noiseutil/chachapoly.go:23-36
 *   neb_decrypt_danger       CipherState.DecryptDanger  noiseutil/cipher_state.go:35,
 *                            noiseutil/aesgcm.go:39-49, noiseutil/chachapoly.go:38-48
 *   neb_overhead             CipherState.Overhead       noiseutil/aesgcm.go:51-56, chachapoly.go:50-55
 *   neb_seal_batch           the per-segment EncryptDanger loop of inside.go:123-146 / :225-236,
 *                            batched at the TX flush point interface.go:465-469,478-487
 *   neb_open_batch           the per-packet ConnectionState.Decrypt → DecryptDanger of
 *                            connection_state.go:99-119 / outside.go:133, batched at the RX flush
 *                            point interface.go:395-400; GMAC-only VerifyRelay
 *                            (connection_state.go:121-148) is an open with len = 0
 *   neb_header_encode/parse  header.Encode header/header.go:102-110, (*H).Parse :143-156
 *   NEB_REJECT_AFTER_MESSAGES noiseutil/cipher_state.go:11-15
 *   neb_window_*             nebula.Bits, the anti-replay window: NewBits bits.go:28-50,
 *                            Check :134-150, Update :152-262, its lost / duplicate / out-of-window
 *                            counters (:23-25, network.packets.{lost,duplicate,out_of_window})
 *   neb_tx_seal_batch        sendInsideMessage's direct branch (inside.go:154-177, :225-239) over a
 *                            batch of TUN reads:
 *                            decodeRead (overlay/tio/tio_gso_linux.go:231-280), SegmentSuperpacket
 *                            (overlay/tio/tun_linux_offload.go:46-60, virtio/segment_linux.go),
 *                            sendInsideEncrypt (inside.go:123-146) into SendBatch slots
 *                            (overlay/batch/tx_batch.go:15-59)
 *   neb_tx_seal_via_batch    the same with its relay branch (inside.go:178-223): the segment
 *                            sealed under the target's key, then prepareSendVia (:442-501)
 *   neb_tx_send_plan         batchWriter.WriteBatch's packing of a SendBatch into sendmmsg entries
 *                            (udp/udp_linux_writebatch.go:194-252) with planRun's UDP_SEGMENT runs
 *                            (:312-346), over the wires of a TX batch
 *   neb_rx_recv_plan         StdConn.ListenOut's split of a recvmmsg batch with UDP_GRO into wire
 *                            packets: getFrom, parseRecvCmsg, deliverSegments (udp/udp_linux.go:237-331)
 *   neb_rx_open_batch_host   ConnectionState.Decrypt (connection_state.go:99-119) over a whole
 *                            receive batch (the recvmmsg flush, interface.go:381-413): window
 *                            Check → DecryptDanger → window Update, results identical to the
 *                            per-packet loop in arrival order
 *   neb_relay_forward_batch  handleOutsideRelayPacket's ForwardingType branch (outside.go:120-130,
 *                            :220-240): VerifyRelay, then SendVia (inside.go:442-501) in place,
 *                            over a whole receive batch
 *   neb_rx_coalesce_batch    MultiCoalescer.Commit / Flush (overlay/batch/multi_coalesce.go:67-133) over a
 *                            whole opened receive batch: the (epoch, counter) sort, the TCP / UDP
 *                            coalescers (tcp_coalesce.go, udp_coalesce.go), Passthrough, and the
 *                            virtio header of every TUN write (overlay/tio/tio_gso_linux.go:280-404);
 *                            neb_rx_plain_from_wire is handleOutsideMessagePacket's hand-over
 *                            (outside.go:145-149, :474-479)
 *   neb_rx_resolve_batch     the lookups readOutsidePackets makes per datagram before it decrypts:
 *                            myVpnNetworksTable.Contains (outside.go:66-74), QueryIndexCached /
 *                            QueryRelayIndex (outside.go:93-106, hostmap.go:546-577) and
 *                            handleOutsideRelayPacket's QueryRelayForByIdx / QueryVpnAddrsRelayFor
 *                            (outside.go:201-240), over neb_index_table_*
 *   neb_rx_inner_batch       handleOutsideMessagePacket between Decrypt and Commit (outside.go:474-494):
 *                            newPacket(out, true, fp) and the two address checks at the head of
 *                            firewall.Drop (firewall.go:425-457), over neb_peer_table_*
 *   neb_queue_*              the flush points themselves (flushSendBatch interface.go:478-487,
 *                            listenOut's flush :395-400) of every routine (interface.go:320-335),
 *                            gathered into shared device batches
 */
#ifndef NEBULA_AEAD_H
#define NEBULA_AEAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NEB_API __attribute__((visibility("default")))

/* Cipher identifiers; the names are the Noise CipherName strings hashed into the handshake. */
#define NEB_ALG_AESGCM 1     /* "AESGCM": AES-256-GCM, nonce 00000000 || BE64(n) (aesgcm.go:31-35) */
#define NEB_ALG_CHACHAPOLY 2 /* "ChaChaPoly": ChaCha20-Poly1305, nonce 00000000 || LE64(n) (chachapoly.go:30-34) */

/* Return codes. */
#define NEB_OK 0
#define NEB_ERR_INVALID (-1)      /* bad argument */
#define NEB_ERR_AUTH (-2)         /* Open: "cipher: message authentication failed"; plaintext region zeroed */
#define NEB_ERR_EXHAUSTED (-3)    /* ErrMessageCounterExhausted (cipher_state.go:18) */
#define NEB_ERR_NO_CIPHER (-4)    /* nil receiver on Encrypt: "no cipher state available to encrypt" */
#define NEB_ERR_SHORT_BUFFER (-5) /* out capacity too small for the appended output */
#define NEB_ERR_HIP (-6)          /* HIP runtime failure */
#define NEB_ERR_NO_DEVICE (-7)    /* no gfx950 device / kernels not loadable */
#define NEB_ERR_NO_KEY_SLOT (-8)  /* key table full */

#define NEB_OVERHEAD 16 /* AEAD tag size (Overhead()) */
#define NEB_HEADER_LEN 16
#define NEB_REJECT_HEADROOM (1ULL << 40)
#define NEB_REJECT_AFTER_MESSAGES (UINT64_MAX - NEB_REJECT_HEADROOM)

/* Per-packet status written by the batch calls. */
#define NEB_STATUS_OK 0
#define NEB_STATUS_AUTH_FAILED 1 /* open: tag mismatch, payload destination zeroed */
#define NEB_STATUS_EXHAUSTED 2   /* seal: counter >= NEB_REJECT_AFTER_MESSAGES, nothing written */
#define NEB_STATUS_BAD_KEY 3     /* key_id not installed / wrong algorithm / violates the uniform-key hint */
#define NEB_STATUS_REPLAY 4      /* receive: the replay window refused the counter — ErrAlreadySeen
                                    (connection_state.go:103-105,114-116); nothing decrypted when
                                    refused before decryption */

typedef struct neb_engine neb_engine; /* one per GPU: stream, key table, staging */
typedef struct neb_cipher neb_cipher; /* one installed tunnel key (a CipherState) */

/* One packet of a batch. Offsets index the batch arena (device memory for neb_*_batch, pinned host
 * memory for neb_*_batch_host).
 *   seal: reads aad[aad_len] at aad_off and pt[len] at src_off; writes ct[len] || tag[16] at dst_off.
 *   open: reads aad at aad_off and ct[len] || tag[16] at src_off; writes pt[len] at dst_off.
 * dst_off == src_off is the in-place form used by Nebula (connection_state.go:107). Any other
 * overlap between one packet's regions, or between packets, is undefined. `counter` is the nonce n
 * (= the header's message counter). */
typedef struct neb_desc {
    uint64_t src_off;
    uint64_t dst_off;
    uint64_t aad_off;
    uint64_t counter;
    uint32_t len;
    uint32_t aad_len;
    uint32_t key_id;
    uint32_t flags; /* reserved, 0 */
} neb_desc;

/* ---- engine ------------------------------------------------------------------------------- */

/* Create an engine on HIP device `device` with room for `max_keys` installed keys. */
NEB_API int neb_engine_create(int device, uint32_t max_keys, neb_engine** out);
NEB_API int neb_engine_destroy(neb_engine* e);
/* Device pointer to the engine's key table and the bytes per key record (for diagnostics). */
NEB_API int neb_engine_info(const neb_engine* e, int* device, uint32_t* max_keys, uint32_t* key_record_bytes);
/* stats[0..3]: slots of the per-packet pool (fixed, 4: streams + pinned staging shared by every
 * thread's neb_encrypt_danger / neb_decrypt_danger), per-packet calls, calls that waited for a
 * slot, keys installed (since creation). */
NEB_API int neb_engine_stats(const neb_engine* e, uint64_t stats[4]);
/* Per-packet AES-256-GCM calls that arrived while every launch slot was busy ride together in one
 * launch (round 6): {such combined launches, calls they carried} since creation. */
NEB_API int neb_engine_pkt_combined(const neb_engine* e, uint64_t out[2]);
/* For tests: n <= 32 per-packet AES-256-GCM requests of one thread as one such combined launch, in
 * the given order (request r rides in slot r of the batch), whatever else is in flight. `in` is the
 * plaintext (seal; out takes in_len + 16 bytes) or the ciphertext and tag (open; out takes
 * in_len - 16). key_id is a raw key slot and counter a raw counter: status[r] is the kernel's own
 * NEB_STATUS_* of request r, and out is written as neb_encrypt_danger / neb_decrypt_danger write it
 * (a failed open: zeros; any other failure: nothing). The batch is one of its own, taken and
 * launched as the combiner does for concurrent calls, which it does not disturb; it counts in
 * neb_engine_pkt_combined. n == 0 is NEB_OK. NEB_ERR_INVALID (nothing launched, nothing written):
 * n > 32, a NULL argument, an open shorter than the tag, or a request the combiner would not take:
 * with pay = ad_len rounded up to 16 it takes pay + in_len <= 2048 and pay + max(in_len, len + 16)
 * <= 2112, len the payload's length without the tag. */
typedef struct neb_pkt_req {
    uint32_t key_id;
    uint32_t reserved;
    uint64_t counter;
    const uint8_t* ad;
    size_t ad_len;
    const uint8_t* in;
    size_t in_len;
    uint8_t* out;
} neb_pkt_req;
NEB_API int neb_engine_pkt_launch(neb_engine* e, int open, const neb_pkt_req* req, uint32_t n, int32_t* status);
/* Every entry point restores the calling thread's current HIP device before it returns. Streams
 * passed to the batch calls must stay alive until the work enqueued on them has completed. */
/* Human-readable text of a return code. */
NEB_API const char* neb_strerror(int rc);
/* Detail of the last NEB_ERR_HIP / NEB_ERR_NO_DEVICE on the calling thread (HIP error string), or of
 * the last multi-engine batch call that fenced key slots (it returns NEB_OK; the fenced packets get
 * NEB_STATUS_BAD_KEY — see neb_cipher_create_multi). */
NEB_API const char* neb_last_error(void);
/* The first 16 hex digits of the SHA-256 of the library's sources (nebula_amd/Makefile SRC then
 * HDR, concatenated) it was built from: a test compares it with the sources beside it. */
NEB_API const char* neb_build_id(void);
/* Measurement: the next device batch this thread launches binds its dominant kernel's begin and end
 * to these two HIP events (hipEvent_t, created with timing enabled) instead of recording markers
 * around it — the single-key kernel, the mixed-key chunk kernel or the ChaCha kernel (a small batch:
 * its one kernel). NULL, NULL disarms. */
NEB_API int neb_time_next_kernel(void* start, void* stop);
/* Process-wide knobs for A/B measurements and tests. Each starts from the environment variable named
 * beside it (read once, at the first use of any knob) and can be changed between batches; batches
 * read them with one atomic load (no getenv on the batch path). */
enum {
    NEB_KNOB_HOST_MODE = 0,       /* NEB_HOST_MODE: 0 zero-copy for mapped arenas (default), 1 "dma" staging */
    NEB_KNOB_SUB_BINS_FROM = 1,   /* NEB_SUB_BINS_FROM: mixed-key batches of at least this many packets
                                   * count their bins in sub-bins (default 262144) */
    NEB_KNOB_SINGLE_MAX_GRID = 2, /* NEB_SINGLE_MAX_GRID: cap on the single-key kernel's workgroups (0: none;
                                   * tests use it to force a partial last pass) */
    NEB_KNOB_RX_STRICT = 3,       /* NEB_RXDEV_STRICT: a device receive whose windows need the sequential host
                                   * finish fails with NEB_ERR_INVALID instead (tests: the parallel form ran) */
    NEB_KNOB_TILE_BINS_FROM = 4,  /* NEB_TILE_BINS_FROM: mixed-key batches of at least this many packets bin
                                   * through per-workgroup LDS histograms (sched.hpp: no per-packet global
                                   * atomic); smaller ones through the atomic histogram */
    NEB_KNOB_SMALL_BATCH = 5,     /* NEB_SMALL_BATCH: a mixed-key AES-GCM batch with fewer packets than this
                                   * per resident wave of the chunk kernel (16 per CU) is chunked finer, up to
                                   * NEB_KNOB_FRONT_GROUPS groups per chunk (default 48; 0: never) */
    NEB_KNOB_FRONT_GROUPS = 6,    /* NEB_FRONT_GROUPS: the 16-packet groups per front chunk of the short size
                                   * classes in such a batch at most (default 1; the classes' own: up to 8) */
    NEB_KNOB_COALESCE_HASH_BITS = 7, /* NEB_COALESCE_HASH_BITS: the device coalescer keeps this many bits of its
                                   * flow hash (default 32; tests force collisions with fewer) */
    NEB_KNOB_COUNT = 8
};
NEB_API int neb_set_knob(int knob, int64_t value);
NEB_API int64_t neb_get_knob(int knob); /* -1 for an unknown knob */
/* The (demangled) name of the kernel the last armed pair was bound to on this thread, or "" when
 * none has been bound yet: what a benchmark's kernel time is the time of. */
NEB_API const char* neb_time_last_kernel(void);

/* ---- key install: noise.CipherFunc.Cipher(k) ----------------------------------------------- */

/* Install a 32-byte key: AES-256 key schedule + H = E_K(0^128) + H^1..H^16 (AESGCM), or the raw
 * ChaCha20 key (ChaChaPoly), computed on the device into the engine's key table. */
NEB_API int neb_cipher_create(neb_engine* e, int alg, const uint8_t key[32], neb_cipher** out);
/* Install n keys at once (keys = n x 32 bytes; out[n]): the tunnel keys a lighthouse or a rekey
 * storm completes in one go (handshake_manager.go:752,877 -> connection_state.go:55-75 per tunnel).
 * One launch of n workgroups and one synchronize instead of n; each key gets the lowest free
 * slot in turn, as n calls of neb_cipher_create would. NEB_ERR_NO_KEY_SLOT (nothing installed)
 * when fewer than n slots are free. */
NEB_API int neb_cipher_create_batch(neb_engine* e, int alg, const uint8_t* keys, uint32_t n, neb_cipher** out);
/* Install ONE tunnel key on every engine of a set (one per GPU; the engines used together by
 * neb_*_batch_host_multi / neb_*_batch_sharded): the same key_id on all of them — the lowest slot
 * free on every engine, reserved on all at once — or on none (NEB_ERR_NO_KEY_SLOT, or the error of
 * the failing engine with the others rolled back). out[k] is the key's cipher on engines[k]; each
 * is destroyed on its own. The installs share one identity that the multi-engine batch calls
 * check (below). A tunnel has exactly one eKey / dKey (connection_state.go:37-49, 55-75). */
NEB_API int neb_cipher_create_multi(neb_engine* const* engines, uint32_t nengines, int alg, const uint8_t key[32],
                                    neb_cipher** out);
/* Waits for the asynchronous batches this engine enqueued that may read the key — the last
 * single-key batch with it on each stream and the last mixed-key batch on each stream — then
 * clears the key record and frees its slot. Other work on the device is not waited for. The caller
 * stops enqueuing batches with the key before destroying it (as Go code stops using a
 * CipherState it drops); a batch enqueued after the destroy gets NEB_STATUS_BAD_KEY for its
 * packets (the kernels check the slot's algorithm tag) or, once the slot is reused, the new key. */
NEB_API int neb_cipher_destroy(neb_cipher* c);
NEB_API uint32_t neb_cipher_key_id(const neb_cipher* c);
NEB_API int neb_cipher_alg(const neb_cipher* c);
NEB_API const char* neb_cipher_name(int alg); /* "AESGCM", "ChaChaPoly", NULL if unknown */

/* ---- per-packet CipherState surface (host buffers; exact Go slice semantics) ---------------- */

/* Overhead(): 16, or 0 when c == NULL. */
NEB_API int neb_overhead(const neb_cipher* c);

/* EncryptDanger(out, ad, plaintext, n, nb): keeps out[0:out_len], appends ct || tag, sets
 * *ret_len = out_len + pt_len + 16. `ad` may alias out[0:out_len] (inside.go:131). `nb` (12 bytes,
 * may be NULL) receives the nonce exactly as the Go code assembles it.
 * Errors: NEB_ERR_NO_CIPHER (c == NULL), NEB_ERR_EXHAUSTED (n >= NEB_REJECT_AFTER_MESSAGES; out
 * untouched), NEB_ERR_SHORT_BUFFER (out_cap < out_len + pt_len + 16). */
NEB_API int neb_encrypt_danger(neb_cipher* c, uint8_t* out, size_t out_len, size_t out_cap, const uint8_t* ad,
                               size_t ad_len, const uint8_t* pt, size_t pt_len, uint64_t n, uint8_t* nb,
                               size_t* ret_len);

/* DecryptDanger(out, ad, ciphertext, n, nb): ciphertext = ct || tag. Keeps out[0:out_len], writes
 * the plaintext after it, *ret_len = out_len + ct_len - 16. In place when out + out_len == ct
 * (connection_state.go:107). On tag mismatch returns NEB_ERR_AUTH, zeroes the would-be plaintext
 * region and touches nothing else (cipher_state_test.go:194-237). c == NULL: returns NEB_OK with
 * *ret_len = 0 (Go returns []byte{}, nil). ct_len < 16 is an auth failure. */
NEB_API int neb_decrypt_danger(neb_cipher* c, uint8_t* out, size_t out_len, size_t out_cap, const uint8_t* ad,
                               size_t ad_len, const uint8_t* ct, size_t ct_len, uint64_t n, uint8_t* nb,
                               size_t* ret_len);

/* ---- batched data plane: device-resident arena ----------------------------------------------- */

/* Key hint for the batch calls: NEB_KEYS_MIXED, or a key_id every descriptor uses (one tunnel's
 * batch) — the engine then keeps that key's round keys in scalar registers and its GHASH tables
 * shared per workgroup. Descriptors whose key_id differs from the hint get NEB_STATUS_BAD_KEY. */
#define NEB_KEYS_MIXED 0xFFFFFFFFu

/* Seal/open n packets. d_desc, d_arena, d_status are device pointers; `stream` is a hipStream_t
 * (NULL = the HIP default stream). Asynchronous: returns after enqueueing. Every descriptor's key must
 * have algorithm `alg`. */
NEB_API int neb_seal_batch(neb_engine* e, int alg, const neb_desc* d_desc, uint32_t n, uint8_t* d_arena,
                           int32_t* d_status, uint32_t key_hint, void* stream);
NEB_API int neb_open_batch(neb_engine* e, int alg, const neb_desc* d_desc, uint32_t n, uint8_t* d_arena,
                           int32_t* d_status, uint32_t key_hint, void* stream);

/* ---- batched data plane: host-resident arena (the TUN / UDP side) ---------------------------- */

/* Same as above but desc/arena/status live in host memory. Synchronous.
 * Every descriptor is first bounds-checked against arena_len, in every mode: an invalid batch
 * returns NEB_ERR_INVALID with the arena and the statuses untouched.
 * - arena pinned and mapped (neb_host_alloc, at any byte address): zero-copy — the kernels load
 *   and store the arena across PCIe directly; desc/status may be pinned or ordinary.
 * - any other arena: the range the descriptors touch is streamed through the device in chunks of
 *   8192 packets, H2D -> kernel -> D2H, rotated over three streams; chunks whose arena ranges
 *   overlap are serialised (each copies its whole range back).
 * Environment, read per call: NEB_HOST_MODE=dma (or NEB_HOST_STAGED=1) stages every arena. */
NEB_API int neb_seal_batch_host(neb_engine* e, int alg, const neb_desc* desc, uint32_t n, uint8_t* arena,
                                size_t arena_len, int32_t* status, uint32_t key_hint);
NEB_API int neb_open_batch_host(neb_engine* e, int alg, const neb_desc* desc, uint32_t n, uint8_t* arena,
                                size_t arena_len, int32_t* status, uint32_t key_hint);

/* ---- several GPUs in one process: contiguous shards, no collective ------------ */
/* Packets are independent, so a batch shards by contiguous packet range over engines (one per GPU,
 * or several on one GPU): shard k takes packets [n*k/m, n*(k+1)/m) of m engines. A batch's keys
 * are engine 0's: install each tunnel key on the set with neb_cipher_create_multi. A packet of
 * shard k whose key_id names a slot where engine k does not hold the same install as engine 0
 * (not installed there, destroyed and reinstalled on one engine, keys installed engine by engine)
 * gets NEB_STATUS_BAD_KEY and is not touched — never sealed or opened with another key. */
/* Host-resident batch (the arena in host memory, pinned or not): one host thread per engine runs
 * neb_seal_batch_host / neb_open_batch_host on its shard; returns when every shard is done, with
 * the first failing shard's return code (the other shards still complete). A staged (not pinned)
 * arena whose shards' byte spans overlap runs the shards one after another. */
NEB_API int neb_seal_batch_host_multi(neb_engine* const* engines, uint32_t nengines, int alg, const neb_desc* desc,
                                      uint32_t n, uint8_t* arena, size_t arena_len, int32_t* status,
                                      uint32_t key_hint);
NEB_API int neb_open_batch_host_multi(neb_engine* const* engines, uint32_t nengines, int alg, const neb_desc* desc,
                                      uint32_t n, uint8_t* arena, size_t arena_len, int32_t* status,
                                      uint32_t key_hint);
/* Device-resident shards: shard k's descriptors, arena and statuses live on engine k's device
 * (each shard's descriptors index its own arena); each is enqueued on its stream (NULL: the
 * device's default stream) and the call returns once every shard is done. */
typedef struct neb_shard {
    neb_engine* e;
    const neb_desc* d_desc;
    uint32_t n;
    uint8_t* d_arena;
    int32_t* d_status;
    void* stream;
} neb_shard;
NEB_API int neb_seal_batch_sharded(int alg, const neb_shard* shards, uint32_t nshards, uint32_t key_hint);
NEB_API int neb_open_batch_sharded(int alg, const neb_shard* shards, uint32_t nshards, uint32_t key_hint);

/* Pinned host memory (hipHostMalloc) for arenas that back the reference's batch.Arena
 * (overlay/batch/coalesce_core.go:142-169) so the batch path needs no bounce copy. */
NEB_API int neb_host_alloc(size_t bytes, void** out);
NEB_API int neb_host_free(void* p);

/* ---- replay window + batched receive ---------------------------------------------------------- */
typedef struct neb_window neb_window; /* one per tunnel (ConnectionState.window, ReplayWindow = 8192) */
/* NewBits(length): length must be a power of two (NEB_ERR_INVALID otherwise; Go panics). */
NEB_API int neb_window_create(uint64_t length, neb_window** out);
NEB_API int neb_window_destroy(neb_window* w);
/* Check(i) / Update(i): 1 = accepted, 0 = refused, < 0 = error. Each call is atomic (the window
 * carries its own lock, ConnectionState.decryptLock). */
NEB_API int neb_window_check(neb_window* w, uint64_t counter);
NEB_API int neb_window_update(neb_window* w, uint64_t counter);
/* current counter and {lost, duplicate, out_of_window} counts since creation / the last reset. */
NEB_API int neb_window_state(const neb_window* w, uint64_t* current, int64_t counters[3]);
NEB_API int neb_window_slot(const neb_window* w, uint64_t slot); /* bit of slot (slot mod length) */
NEB_API int neb_window_reset_counters(neb_window* w);
/* Receive a batch in arrival order: for every packet, windows[desc.key_id] (NULL or key_id >=
 * nwindows → NEB_STATUS_BAD_KEY) is checked, the packet opened in place (host arena, as
 * neb_open_batch_host) and the window updated — statuses OK / AUTH_FAILED / BAD_KEY / REPLAY,
 * window contents and counters identical to calling Decrypt packet by packet. All packets that
 * pass go to the GPU as one batch; a packet refused by its window is not decrypted. */
NEB_API int neb_rx_open_batch_host(neb_engine* e, int alg, neb_window* const* windows, uint32_t nwindows,
                                   const neb_desc* desc, uint32_t n, uint8_t* arena, size_t arena_len,
                                   int32_t* status, uint32_t key_hint);
/* Replay windows in device memory, for receive batches that stay on the device (neb_rx_open_batch).
 * A set holds `count` windows of one power-of-two length, all absent at creation. load copies a
 * host window's state into slot idx (NULL: the slot becomes absent); store copies slot idx back
 * into a host window of the same length (NEB_ERR_INVALID for an absent slot). Synchronous. */
typedef struct neb_dwindows neb_dwindows;
NEB_API int neb_dwindows_create(neb_engine* e, uint32_t count, uint64_t length, neb_dwindows** out);
NEB_API int neb_dwindows_destroy(neb_dwindows* d);
NEB_API int neb_dwindows_load(neb_dwindows* d, uint32_t idx, const neb_window* w);
NEB_API int neb_dwindows_store(neb_dwindows* d, uint32_t idx, neb_window* w);
/* Fault injection for tests: the polls a device receive's scan may spend waiting for an earlier
 * workgroup before the batch fails with NEB_ERR_HIP (default 2^20, about 0.1 s; 0 fails every scan
 * that has to wait). A failed batch moves no window. */
NEB_API int neb_dwindows_set_spin_limit(neb_dwindows* d, uint32_t limit);
/* neb_rx_open_batch_host over a device-resident batch (device descriptors, arena and statuses),
 * with the windows of `d` (slot desc.key_id; absent or out of range → NEB_STATUS_BAD_KEY): the
 * same statuses, arena bytes, window contents and counters as Decrypt packet by packet. Runs on
 * `stream` and returns when the batch is done (it reads back which windows need the exact
 * sequential finish: those where a tag failed, or counters within 2^62 of wrapping). */
NEB_API int neb_rx_open_batch(neb_engine* e, int alg, neb_dwindows* d, const neb_desc* d_desc, uint32_t n,
                              uint8_t* d_arena, int32_t* d_status, uint32_t key_hint, void* stream);
/* ---- receive from the wire: readOutsidePackets' gate in front of Decrypt / VerifyRelay ---------- */
/* One received UDP datagram (or GRO segment) of a receive batch, as readOutsidePackets gets it
 * (outside.go:30): the wire packet header(16) || ct || tag(16) at off of the arena, len bytes, and
 * the tunnel (window / key slot) the caller's hostmap lookup resolved from the header's remote
 * index (outside.go:94-100), NEB_KEYS_MIXED when it found none. */
typedef struct neb_rx_packet {
    uint64_t off;
    uint32_t len;
    uint32_t key_id;
} neb_rx_packet;
#define NEB_STATUS_NOT_MESSAGE 7 /* a valid header of an unencrypted type (handshake, recv error,
                                    outside.go:83-89): left to the control plane, untouched */
/* Or-ed into neb_rx_packet.len by the caller for a datagram that readOutsidePackets' double-
 * encryption check refuses (outside.go:66-74: not relayed, and the UDP source address is inside the
 * node's own VPN networks, f.myVpnNetworksTable). The batch does not carry source addresses, so the
 * caller makes that lookup; the gate then drops the packet as the reference does, right after
 * IsValidSubType and before the handshake hand-off: NEB_STATUS_INVALID, nothing touched. */
#define NEB_RX_OWN_SOURCE 0x80000000u
/* Per packet, readOutsidePackets up to the decrypt, then Decrypt or VerifyRelay: h.Parse (len < 16:
 * NEB_STATUS_INVALID, header.go:143-146); version 1 and IsValidSubType (header.go:192-205), else
 * NEB_STATUS_INVALID (outside.go:49-64); Handshake / RecvError types -> NEB_STATUS_NOT_MESSAGE; no
 * tunnel -> NEB_STATUS_BAD_KEY (outside.go:100-106); len < 16 + 16 -> NEB_STATUS_INVALID
 * (outside.go:108-114); the nonce is the header's counter (bytes 8:16, big-endian). Message/Relay
 * packets are verified GMAC-only over packet[:len-16] (VerifyRelay, connection_state.go:121-148),
 * every other type is opened in place with the header as AAD (Decrypt, connection_state.go:99-119),
 * both through the replay window of their tunnel: statuses, arena bytes and windows as
 * neb_rx_open_batch_host / neb_rx_open_batch give for the descriptors the gate builds. Packets the
 * gate refuses are not touched. The host form checks every packet against arena_len first. */
NEB_API int neb_rx_open_wire_batch_host(neb_engine* e, int alg, neb_window* const* windows, uint32_t nwindows,
                                        const neb_rx_packet* pk, uint32_t n, uint8_t* arena, size_t arena_len,
                                        int32_t* status, uint32_t key_hint);
NEB_API int neb_rx_open_wire_batch(neb_engine* e, int alg, neb_dwindows* d, const neb_rx_packet* d_pk, uint32_t n,
                                   uint8_t* d_arena, int32_t* d_status, uint32_t key_hint, void* stream);
/* ---- transmit: TUN reads (IP packets, TSO/USO superpackets) -> sealed wire packets ------------ */
/* virtio_net_hdr values (linux/virtio_net.h), as the TUN hands them over (overlay/tio/virtio/header_linux.go) */
#define NEB_VNET_F_NEEDS_CSUM 1
#define NEB_VNET_F_RSC_INFO 4
#define NEB_GSO_NONE 0
#define NEB_GSO_TCPV4 1
#define NEB_GSO_TCPV6 4
#define NEB_GSO_UDP_L4 5
#define NEB_GSO_ECN 0x80
/* Per-packet status of a TX batch (besides NEB_STATUS_OK / NEB_STATUS_BAD_KEY = the tunnel has no
 * key, `if ci.eKey == nil { return }`, inside.go:155-158). */
#define NEB_STATUS_INVALID 5  /* virtio / IP header rejected (decodeRead, CheckValid, CorrectHdrLen,
                                 SegmentTCP/UDP, FinishChecksum errors): dropped, no counter used */
#define NEB_STATUS_NO_SPACE 6 /* the output arena or the wire array is full: dropped */
/* One TUN read: an IP packet at in_off of the input arena with its virtio_net_hdr, bound for a tunnel. */
typedef struct neb_tx_packet {
    uint64_t in_off;
    uint32_t len;
    uint32_t tunnel;     /* index into the tunnel array */
    uint8_t vnet_flags;  /* virtio_net_hdr.flags */
    uint8_t gso_type;    /* virtio_net_hdr.gso_type (the ECN qualifier allowed) */
    uint16_t hdr_len;    /* virtio_net_hdr.hdr_len (re-derived from the TCP header, CorrectHdrLen) */
    uint16_t gso_size;
    uint16_t csum_start;
    uint16_t csum_offset;
    uint16_t reserved;
} neb_tx_packet;
/* The sending side of one tunnel (ConnectionState + HostInfo fields the TX path reads). */
typedef struct neb_tx_tunnel {
    uint64_t message_counter; /* ConnectionState.messageCounter: the last counter used; the batch
                                 advances it by one per segment, as inside.go:127 does */
    uint32_t key_id;          /* the eKey's key_id (neb_cipher_key_id); NEB_KEYS_MIXED = no eKey */
    uint32_t remote_index;    /* hostinfo.remoteIndexId, written into every header */
} neb_tx_tunnel;
/* One wire packet: header(16) || ct || tag(16) at out_off (16-byte aligned) of the output arena. */
typedef struct neb_tx_wire {
    uint64_t out_off;
    uint64_t counter;
    uint32_t len;     /* 16 + segment + 16 */
    uint32_t packet;  /* index of the neb_tx_packet it came from */
    uint32_t segment; /* segment index within that packet */
    uint32_t reserved; /* neb_tx_seal_via_batch: NEB_TX_WIRE_VIA for a wire sent through a relay, else 0 */
} neb_tx_wire;
#define NEB_TX_WIRE_VIA 1
/* sendInsideMessage's direct branch (inside.go:154-177 and :225-239; the relay branch :178-223 is
 * neb_tx_seal_via_batch below) for a whole batch of TUN reads: every packet is validated
 * and segmented exactly as decodeRead + SegmentSuperpacket do (TSO: per-segment seq, CWR/FIN/PSH,
 * IPv4 ID and lengths, IPv4 and TCP checksums; USO: lengths and UDP checksum; plain packets with
 * NEEDS_CSUM get FinishChecksum), each segment takes the next counter of its tunnel in batch order,
 * gets header.Encode(Message, remote_index, counter) and is sealed into its output slot (the seal
 * reads the payload straight from d_in, which must stay valid until the stream has run the batch;
 * only the patched L3/L4 headers are written into the slot first): wires[i] describes the
 * i-th segment of the batch (packet order, then segment order), wire_status[i] is its seal status
 * (NEB_STATUS_EXHAUSTED = dropped, inside.go:137-145, its counter still used). The segment count is
 * written to *d_nwires. Device pointers; asynchronous on `stream`. tunnels[].message_counter is
 * advanced on the device. */
NEB_API int neb_tx_seal_batch(neb_engine* e, int alg, neb_tx_tunnel* d_tunnels, uint32_t ntunnels,
                              const neb_tx_packet* d_packets, uint32_t npackets, const uint8_t* d_in,
                              uint8_t* d_out, size_t out_cap, neb_tx_wire* d_wires, int32_t* d_wire_status,
                              uint32_t max_wires, uint32_t* d_nwires, int32_t* d_packet_status, uint32_t key_hint,
                              void* stream);
/* The same over host memory (synchronous): the input span is uploaded, the outputs downloaded. */
NEB_API int neb_tx_seal_batch_host(neb_engine* e, int alg, neb_tx_tunnel* tunnels, uint32_t ntunnels,
                                   const neb_tx_packet* packets, uint32_t npackets, const uint8_t* in, size_t in_len,
                                   uint8_t* out, size_t out_cap, neb_tx_wire* wires, int32_t* wire_status,
                                   uint32_t max_wires, uint32_t* nwires, int32_t* packet_status, uint32_t key_hint);
/* ---- relay forwarding: VerifyRelay, then SendVia in place ------------------------------------- */
/* A relay node forwards every relayed packet the same way (handleOutsideRelayPacket's ForwardingType
 * branch, outside.go:120-130 and :220-240; SendVia, inside.go:442-501): VerifyRelay with the inbound
 * tunnel's key through its replay window, the next message counter of the outbound tunnel, a new
 * Message/Relay header over the old one and a new tag under the outbound key where the old tag
 * was — one packet at a time ("it would potentially be nice to batch these", outside.go:239).
 * These calls do it for a whole receive batch. TerminalType relays (the inner packet is for this
 * node) are not unwrapped here: the caller gives them no route and receives them with
 * neb_rx_open_via_batch (below), which verifies, unwraps and opens them in one call. */
#define NEB_RELAY_NONE 0xFFFFFFFFu
#define NEB_STATUS_NOT_FORWARDED 8 /* fwd_status: not a verified Message/Relay packet, or no route */
/* Per received packet: what the caller's relay lookups found for the header's remote index
 * (relayState.QueryRelayForByIdx, outside.go:201, then hostMap.QueryVpnAddrsRelayFor, :222; a route
 * only for an Established ForwardingType target, :233-240). */
typedef struct neb_relay_route {
    uint32_t tunnel;       /* index into the tunnel array (the target HostInfo); NEB_RELAY_NONE: do not forward */
    uint32_t remote_index; /* targetRelay.RemoteIndex, written into the new header (inside.go:462) */
} neb_relay_route;
/* Receive half: status[], the arena and the windows are exactly what neb_rx_open_wire_batch[_host]
 * gives for the same pk (the gate, replay and tag statuses, other packets opened in place, all in
 * arrival order); key_hint applies to it.
 * Forward half, per packet i in arrival order. Eligible: status[i] == NEB_STATUS_OK, the header is
 * Message/Relay (type 1, subtype 1) and route[i].tunnel != NEB_RELAY_NONE; every other packet gets
 * fwd_status[i] = NEB_STATUS_NOT_FORWARDED, no further write and no counter. NEB_STATUS_BAD_KEY:
 * route[i].tunnel >= ntunnels, or that tunnel's key_id is NEB_KEYS_MIXED, not installed, or of the
 * other algorithm (no usable eKey, as neb_tx_seal_batch's NEB_STATUS_BAD_KEY): untouched, no counter. Otherwise the packet takes the next
 * counter of tunnels[t]: the k-th such packet of tunnel t in arrival order gets message_counter + k
 * (k from 1); a forgery or a replay between two valid packets takes none, as the reference
 * allocates only after VerifyRelay returned nil. A counter >= NEB_REJECT_AFTER_MESSAGES:
 * NEB_STATUS_EXHAUSTED, the packet untouched (prepareSendVia returns before Encode), the counter
 * still used, as neb_tx_seal_batch does for a segment. Otherwise NEB_STATUS_OK: bytes 0..15 become
 * header.Encode(1, Message, MessageRelay, route[i].remote_index, c), bytes len-16..len the tag of
 * the AD-only seal under the tunnel's key with nonce c over packet[:len-16] (with the new header);
 * the bytes in between are not written. tunnels[].message_counter advances by the counters taken
 * (on the device for the device form, so forwarding and neb_tx_seal_batch on the same array and
 * stream share the counters; the host form updates the caller's array).
 * Device form: device pointers; returns once the receive is done, with the forward half enqueued
 * on `stream`: every output is valid once `stream` is synchronized. With ntunnels == 1 the
 * forwarding seal runs as a single-key batch. ChaCha20-Poly1305 tags are Poly1305 over the AD, as
 * VerifyRelay's. A packet whose target key is destroyed while the batch runs may get the seal's
 * NEB_STATUS_BAD_KEY with its header already rewritten. */
NEB_API int neb_relay_forward_batch(neb_engine* e, int alg, neb_dwindows* d, const neb_rx_packet* d_pk,
                                    const neb_relay_route* d_route, uint32_t n, neb_tx_tunnel* d_tunnels,
                                    uint32_t ntunnels, uint8_t* d_arena, int32_t* d_status, int32_t* d_fwd_status,
                                    uint32_t key_hint, void* stream);
/* The same over host memory (synchronous; arena as neb_rx_open_wire_batch_host's). */
NEB_API int neb_relay_forward_batch_host(neb_engine* e, int alg, neb_window* const* windows, uint32_t nwindows,
                                         const neb_rx_packet* pk, const neb_relay_route* route, uint32_t n,
                                         neb_tx_tunnel* tunnels, uint32_t ntunnels, uint8_t* arena, size_t arena_len,
                                         int32_t* status, int32_t* fwd_status, uint32_t key_hint);
/* ---- receive through a relay: VerifyRelay, then unwrap and open, in one call --------------------- */
/* A node reached through a relay gets every data packet wrapped: handleOutsideRelayPacket's
 * TerminalType branch (outside.go:191-219) runs VerifyRelay on the outer packet through the relay
 * tunnel's window, strips the outer header and tag (signedPayload = packet[16 : len-16]) and calls
 * readOutsidePackets again on the inner packet with IsRelayed = true. These calls do both levels
 * for a whole receive batch. */
#define NEB_VIA_TERMINAL 1       /* relay.Type == TerminalType for the outer header's remote index
                                    (relayState.QueryRelayForByIdx, outside.go:201-210) */
#define NEB_STATUS_NOT_RELAYED 9 /* inner_status: no inner packet (not a verified terminal relay packet) */
typedef struct neb_rx_via {      /* per received datagram, the caller's lookups for the INNER packet */
    uint32_t key_id; /* tunnel resolved from the inner header's remote index (the header at off+16;
                        the caller may look it up before anything is verified: it is used only if the
                        outer packet verifies); NEB_KEYS_MIXED: none */
    uint32_t flags;  /* NEB_VIA_TERMINAL */
} neb_rx_via;
/* Phase 1 (outer): status[], the arena and the windows are exactly what
 * neb_rx_open_wire_batch[_host] gives for the same pk; key_hint applies to it.
 * Unwrap, per packet i. Eligible: status[i] == NEB_STATUS_OK, the header is Message/Relay (type 1,
 * subtype 1) and via[i].flags & NEB_VIA_TERMINAL. An eligible packet gets inner_pk[i] = {pk[i].off +
 * 16, len - 32, via[i].key_id} (len without NEB_RX_OWN_SOURCE, which an inner record never carries:
 * IsRelayed skips that check, outside.go:66). Every other packet gets inner_pk[i] = {pk[i].off, 0,
 * NEB_KEYS_MIXED} and inner_status[i] = NEB_STATUS_NOT_RELAYED, no further write and no window event.
 * Phase 2 (inner): the wire receive of neb_rx_open_wire_batch over inner_pk[] in arrival order
 * writes inner_status[]: the same gate, windows and in-place open, with inner_key_hint. So an inner
 * Decrypt opens in place at pk[i].off + 32 (the outer header, the inner header and the outer tag are
 * not written); an inner packet shorter than 16 or than 32 bytes, hole punches among them, gets
 * NEB_STATUS_INVALID, one with no tunnel NEB_STATUS_BAD_KEY, an inner handshake or recv error
 * NEB_STATUS_NOT_MESSAGE. One exception to the gate: an inner packet that is itself Message/Relay
 * (checked where the gate hands over the unencrypted types) is not verified and takes no window
 * event: NEB_STATUS_NOT_MESSAGE, untouched, for the caller to feed into another call. That is one
 * level of the reference's recursion per call; no sender produces nesting, a relay is always
 * reached directly (inside.go:183-198).
 * Order. The batch is the reference's loop with the recursion deferred: every datagram's own gate,
 * Check, verify and Update run first, in arrival order; the recursive call of every terminal relay
 * packet that verified runs afterwards, in arrival order. That equals the strict per-packet
 * recursion whenever no tunnel takes a window event in both phases of one batch. Where one does (a
 * peer heard directly and through a relay in the same batch), the outcome is the strict loop's for
 * an arrival order with the direct packets first.
 * inner_pk and inner_status are index-aligned with pk and go unchanged into neb_rx_plain_from_wire
 * and neb_rx_coalesce_batch. n == 0 returns NEB_OK.
 * Device form: device pointers; d->mu is held across both phases and the call returns with `stream`
 * synchronized, as neb_rx_open_wire_batch does. A batch without an eligible packet costs one kernel
 * in place of neb_rx_open_wire_batch's last and nothing more. */
NEB_API int neb_rx_open_via_batch(neb_engine* e, int alg, neb_dwindows* d, const neb_rx_packet* d_pk,
                                  const neb_rx_via* d_via, uint32_t n, uint8_t* d_arena, int32_t* d_status,
                                  neb_rx_packet* d_inner_pk, int32_t* d_inner_status, uint32_t key_hint,
                                  uint32_t inner_key_hint, void* stream);
/* The same over host memory (synchronous); every pk is checked against arena_len first
 * (NEB_ERR_INVALID: nothing written). */
NEB_API int neb_rx_open_via_batch_host(neb_engine* e, int alg, neb_window* const* windows, uint32_t nwindows,
                                       const neb_rx_packet* pk, const neb_rx_via* via, uint32_t n, uint8_t* arena,
                                       size_t arena_len, int32_t* status, neb_rx_packet* inner_pk,
                                       int32_t* inner_status, uint32_t key_hint, uint32_t inner_key_hint);
/* The unwrap rule alone, on the CPU (no engine): inner_pk[] and, for the packets that are not
 * eligible, inner_status[] = NEB_STATUS_NOT_RELAYED; an eligible packet's inner_status is set to
 * NEB_STATUS_OK, to be overwritten by the receive of inner_pk. Every pk is checked against arena_len
 * first (NEB_ERR_INVALID: nothing written). */
NEB_API int neb_rx_via_unwrap_host(const neb_rx_packet* pk, const neb_rx_via* via, const int32_t* status, uint32_t n,
                                   const uint8_t* arena, size_t arena_len, neb_rx_packet* inner_pk,
                                   int32_t* inner_status);
/* ---- transmit through a relay: seal, then SendVia, in one call ---------------------------------- */
/* sendInsideMessage with its relay branch (inside.go:178-223: `!remote.IsValid()`, the target is
 * reached only through a relay): neb_tx_seal_batch[_host] plus via[0..ntunnels). via[t].tunnel is
 * the index, in the same tunnel array, of the relay tunnel of target tunnel t (relayHostInfo of
 * QueryVpnAddrsRelayFor, inside.go:183-198), via[t].remote_index is relay.RemoteIndex
 * (inside.go:462); NEB_RELAY_NONE: t is sent directly. via == NULL: every tunnel is direct, the
 * call is neb_tx_seal_batch.
 * Per TUN read i in batch order, t = packets[i].tunnel, v = via[t].tunnel: validation, BAD_KEY for
 * t and the fitting prefix (NO_SPACE) as neb_tx_seal_batch, except that a via segment's slot is
 * (16 + 16 + seg + 16 + 16) rounded up to 16. With v != NEB_RELAY_NONE, after t's key check and
 * before segment-time validation: v >= ntunnels or tunnel v without a usable key of this algorithm
 * -> packet_status NEB_STATUS_BAD_KEY (no relay found: the reference returns before
 * SegmentSuperpacket, inside.go:195-198); v == t or via[v].tunnel != NEB_RELAY_NONE (a relay is
 * always reached directly: the reference sends to relayHostInfo.GetRemote()) -> NEB_STATUS_INVALID;
 * either way no wire and no counter on any tunnel.
 * Segment j of a via read takes the next counter c of tunnel t (inside.go:127); its slot holds at
 * +16 header.Encode(1, Message, 0, tunnels[t].remote_index, c), at +32 the ciphertext, then the
 * inner tag: the direct wire of the same counter. c >= NEB_REJECT_AFTER_MESSAGES: wire_status
 * NEB_STATUS_EXHAUSTED, c still used, no counter of v (sendInsideEncrypt returns nil before
 * prepareSendVia, inside.go:204-207). Otherwise the segment takes the next counter r of tunnel v
 * (prepareSendVia, inside.go:442-501); r >= NEB_REJECT_AFTER_MESSAGES: NEB_STATUS_EXHAUSTED, r still
 * used (neb_relay_forward_batch's rule). Otherwise bytes 0..15 of the slot are
 * header.Encode(1, Message, MessageRelay, via[t].remote_index, r), the last 16 bytes the tag of the
 * AD-only seal under v's key with nonce r over slot[0 : 48 + seg], and wires[].len = seg + 64. The
 * bytes of a dropped slot are unspecified. wires[].counter is the inner counter c; wires[].reserved
 * is NEB_TX_WIRE_VIA for a via wire (send it to the relay's remote) and 0 for a direct one. Direct
 * reads of the batch behave as in neb_tx_seal_batch.
 * Counters: tunnel v hands out message_counter + 1, + 2, ... in batch order (packet, then segment)
 * to its own direct segments and to the outer headers of the via segments routed through it whose
 * inner counter was not exhausted. tunnels[].message_counter advances on the device by the
 * counters taken, so a via batch, neb_tx_seal_batch and neb_relay_forward_batch on one tunnel array
 * and stream share the counters without gaps or repeats.
 * key_hint applies to the inner seal (the targets' keys). The outer AD-only seal is a second pass
 * on the same stream; it runs as a single-key batch when every relay tunnel named in via has the
 * same key. The device form reads that one word back while the batch runs (it waits for the work
 * queued on `stream` before this call, not for the batch). A via wire whose relay key is destroyed
 * while the batch runs may get the outer seal's NEB_STATUS_BAD_KEY. */
NEB_API int neb_tx_seal_via_batch(neb_engine* e, int alg, neb_tx_tunnel* d_tunnels, uint32_t ntunnels,
                                  const neb_relay_route* d_via, const neb_tx_packet* d_packets, uint32_t npackets,
                                  const uint8_t* d_in, uint8_t* d_out, size_t out_cap, neb_tx_wire* d_wires,
                                  int32_t* d_wire_status, uint32_t max_wires, uint32_t* d_nwires,
                                  int32_t* d_packet_status, uint32_t key_hint, void* stream);
/* The same over host memory (synchronous); via is uploaded beside the tunnels. */
NEB_API int neb_tx_seal_via_batch_host(neb_engine* e, int alg, neb_tx_tunnel* tunnels, uint32_t ntunnels,
                                       const neb_relay_route* via, const neb_tx_packet* packets, uint32_t npackets,
                                       const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap,
                                       neb_tx_wire* wires, int32_t* wire_status, uint32_t max_wires,
                                       uint32_t* nwires, int32_t* packet_status, uint32_t key_hint);
/* ---- TX send plan: sealed wires -> sendmmsg entries with UDP_SEGMENT runs ------------------------ */
/* What batchWriter.WriteBatch does with a SendBatch before it calls sendmmsg
 * (udp/udp_linux_writebatch.go:194-252, planRun :312-346), for the wires of a TX batch: consecutive
 * packets to one destination become UDP_SEGMENT runs (equal sizes, a shorter packet only as the
 * last; at most max_segments packets and NEB_SEND_MAX_BYTES bytes), destinations the socket cannot
 * address are skipped, and the iovecs are packed into chunks of chunk_packets. The plan only names
 * bytes: the caller builds mmsghdr, iovec and cmsg from it and sends. */
#define NEB_STATUS_UNROUTABLE 16 /* send_status: the socket cannot address the destination: skipped */
#define NEB_STATUS_NOT_SENT 17   /* send_status: wire_status != OK (never committed to the SendBatch) */
#define NEB_SEND_NONE 0xFFFFFFFFu
#define NEB_SEND_MAX_BYTES 65000 /* maxGSOBytes */
typedef struct neb_udp_addr {    /* netip.AddrPort of hostinfo.remote; compared as these 20 bytes */
    uint8_t addr[16];            /* family 4: addr[0..4), the rest 0 */
    uint16_t port;
    uint8_t family;              /* 0: no valid remote; 4; 6 */
    uint8_t reserved;            /* 0 */
} neb_udp_addr;
typedef struct neb_send_iov { uint64_t off; uint32_t len; uint32_t wire; } neb_send_iov;   /* one iovec */
typedef struct neb_send_entry {  /* one mmsghdr */
    uint32_t iov_first;          /* iov[iov_first .. iov_first + niov) */
    uint16_t niov;
    uint16_t seg_size;           /* UDP_SEGMENT cmsg payload; 0 = no cmsg (niov == 1) */
    uint32_t dst;                /* tunnel index whose remote[] is msg_name */
    uint32_t bytes;              /* sum of the iov lengths */
} neb_send_entry;
/* Per wire i < *d_nwires, in wire order:
 *   wire_status[i] != NEB_STATUS_OK: the packet was never committed (inside.go:137-145):
 *   send_status[i] = NEB_STATUS_NOT_SENT, it is absent from the plan, and a run continues across it;
 *   its destination tunnel is t = packets[wires[i].packet].tunnel, or via[t].tunnel when
 *   wires[i].reserved has NEB_TX_WIRE_VIA (relayHostInfo.GetRemote(), inside.go:216). A packet
 *   index >= npackets, a tunnel index >= ntunnels or a via index >= ntunnels (checked in that order;
 *   a via wire with via == NULL counts as the last): NEB_STATUS_BAD_KEY; the wire is then unroutable
 *   with a destination of its own, so it breaks runs;
 *   remote[t] not addressable by the socket: NEB_STATUS_UNROUTABLE, in no entry. Family 4 is always
 *   addressable; family 6 on a v6 socket (socket_v4 == 0), and on a v4 socket when the address is in
 *   ::ffff:0:0/96 (Unmap, udp_linux.go:371-376). Any other family is not. Deviation: family 0 (no
 *   valid remote) is unroutable on either socket, where the reference never commits a packet to an
 *   invalid direct remote at all (inside.go:178). Unroutable wires take no iovec, but they are
 *   among WriteBatch's bufs and break runs, because their destination differs;
 *   otherwise NEB_STATUS_OK: the wire is in exactly one entry, wire_entry[i]; every other wire has
 *   wire_entry[i] = NEB_SEND_NONE.
 * The wires that are not NOT_SENT are WriteBatch's bufs with addrs[] = remote[t] (compared as 20
 * bytes), and planRun applies with maxGSOSegments = max_segments (<= 1: GSO is off, every packet is
 * its own entry) and maxGSOBytes = NEB_SEND_MAX_BYTES: a packet of size 0 or above the byte cap is a
 * run of one; a next packet that is empty, longer, to another destination or past a cap ends the
 * run; a shorter one joins the run and ends it.
 * Chunks: a chunk holds chunk_packets iovecs (the reference's scratch has 128; 0 = unlimited) and no
 * run crosses a chunk. Skipped runs use no iovec, so chunk c is exactly
 * iov[c * chunk_packets .. (c + 1) * chunk_packets): the entries of one sendmmsg call are those whose
 * iov_first lies in that span, and the caller derives each call's span from iov_first alone.
 * Entries are in wire order. seg_size is the first packet's length when niov >= 2, else 0; dst is
 * the first wire's destination tunnel; iov[k] is {wires[w].out_off, wires[w].len, w}. *niov and
 * *nentries get the counts. iov, entries, wire_entry and send_status hold max_wires elements each,
 * which nothing can overflow; elements past the counts (past *d_nwires for the per-wire arrays) are
 * not written.
 * Device pointers (d_iov 8-byte, d_remote and the others 4-byte aligned); asynchronous on `stream`:
 * *d_nwires (clamped to max_wires) is read on the device, with no read-back and no synchronisation,
 * so the call can follow neb_tx_seal_batch / neb_tx_seal_via_batch on their stream directly. Its cost
 * follows max_wires, not *d_nwires. max_wires == 0 returns NEB_OK and writes nothing.
 * NEB_ERR_INVALID: max_segments > 1024, or a required array is NULL (every one but d_via; d_packets
 * and d_remote may be NULL when their count is 0).
 * Not part of the plan: resuming a partial send, and the EIO path that disables GSO and replays:
 * after an EIO on an entry with niov >= 2 the caller plans again with max_segments = 1. */
NEB_API int neb_tx_send_plan(neb_engine* e, const neb_tx_wire* d_wires, const int32_t* d_wire_status,
                             const uint32_t* d_nwires, uint32_t max_wires, const neb_tx_packet* d_packets,
                             uint32_t npackets, const neb_relay_route* d_via /* may be NULL */,
                             const neb_udp_addr* d_remote, uint32_t ntunnels, uint32_t socket_v4,
                             uint32_t max_segments, uint32_t chunk_packets, neb_send_iov* d_iov, uint32_t* d_niov,
                             neb_send_entry* d_entries, uint32_t* d_nentries, uint32_t* d_wire_entry,
                             int32_t* d_send_status, void* stream);
/* The same over host memory with nwires by value: the plain sequential loop, no engine, no GPU. The
 * four output arrays hold nwires elements. */
NEB_API int neb_tx_send_plan_host(const neb_tx_wire* wires, const int32_t* wire_status, uint32_t nwires,
                                  const neb_tx_packet* packets, uint32_t npackets,
                                  const neb_relay_route* via /* may be NULL */, const neb_udp_addr* remote,
                                  uint32_t ntunnels, uint32_t socket_v4, uint32_t max_segments,
                                  uint32_t chunk_packets, neb_send_iov* iov, uint32_t* niov,
                                  neb_send_entry* entries, uint32_t* nentries, uint32_t* wire_entry,
                                  int32_t* send_status);
/* ---- receive: opened packets -> TUN writes (TSO / USO superpackets) ---------------------------- */
/* What the reference does between the open and the TUN write: MultiCoalescer.Commit per packet, then
 * Flush (overlay/batch/multi_coalesce.go): sort by (epoch, counter), coalesce in-flow TCP / UDP runs
 * into superpackets, pass everything else through, and give every write its virtio_net_hdr. */
#define NEB_VNET_F_DATA_VALID 2
#define NEB_PLAIN_PARSED 1   /* proto / ip_hdr_len / FRAG_ANY are the caller's firewall parse
                                (firewall.ParsedPacket); else they are derived as newPacket does */
#define NEB_PLAIN_FRAG_ANY 2 /* ParsedPacket.FragAny (with NEB_PLAIN_PARSED) */
#define NEB_PLAIN_SKIP 4     /* not committed (firewall drop, not a data message, not opened) */
typedef struct neb_plain_packet { /* one MultiCoalescer.Commit */
    uint64_t off;     /* the plaintext IP packet in the input arena */
    uint64_t epoch;   /* SortKey.Epoch */
    uint64_t counter; /* SortKey.Counter */
    uint32_t len;
    uint16_t ip_hdr_len;
    uint8_t proto;
    uint8_t flags; /* NEB_PLAIN_* */
} neb_plain_packet;
typedef struct neb_tun_write { /* one write to the TUN, in the reference's emission order */
    uint64_t out_off; /* 16-byte aligned, in the output arena */
    uint32_t len;
    uint32_t first; /* input index of the verbatim packet / the chain's seed */
    uint16_t nseg;  /* packets it carries (1 for verbatim) */
    uint8_t vnet_flags, gso_type;
    uint16_t hdr_len, gso_size, csum_start, csum_offset;
    uint8_t lane; /* 0 TCP, 1 UDP, 2 passthrough */
    uint8_t reserved[3];
} neb_tun_write;
#define NEB_COALESCE_TCP 1 /* the TUN accepts TSO writes (tio.Capabilities.TSO) */
#define NEB_COALESCE_UDP 2 /* ... USO */
#define NEB_WRITE_NONE 0xFFFFFFFFu
/* MultiCoalescer.Flush over the records without NEB_PLAIN_SKIP.
 * A record whose derived parse (newPacket, outside.go:320-472) fails, or an empty packet, is dropped:
 * pkt_status NEB_STATUS_INVALID, it takes part in nothing. The others are sorted by (epoch, counter),
 * ties by input index. Protocol 6 goes to the TCP lane if lanes & NEB_COALESCE_TCP, 17 to the UDP lane
 * if lanes & NEB_COALESCE_UDP, everything else to passthrough. Writes come in the reference's order:
 * the TCP lane's slots in creation order (the sorted position of the verbatim packet or the seed),
 * then the UDP lane's, then the passthrough packets in sorted order. A verbatim slot or a chain that
 * stayed at one segment is the whole input packet, untrimmed, with vnet_flags DATA_VALID and every
 * other field 0. A chain of >= 2 segments is the seed's hdr_len header bytes patched as flushSlot
 * does (lengths, IPv4 header checksum, the folded pseudo-header sum in the L4 checksum field, PSH
 * of an appended segment or-ed in) followed by the trimmed payloads in chain order, with NEEDS_CSUM,
 * gso_type TCPV4 / TCPV6 / UDP_L4, hdr_len, gso_size = the seed's payload length, csum_start = the
 * IP header length and csum_offset 16 / 6. The input arena is only read (the reference patches the
 * seed in place; this call does not). Writes are placed in order at 16-byte aligned offsets; the
 * longest prefix that fits out_cap and max_writes is emitted and counted in *nwrites, the packets of
 * the writes cut off get NEB_STATUS_NO_SPACE. pkt_write[i] is the write that carries packet i or
 * NEB_WRITE_NONE; pkt_status[i] is NEB_STATUS_OK, _INVALID, _NO_SPACE or, for a skipped record,
 * NEB_STATUS_NOT_MESSAGE. Flow identity is the full 38-byte key {src, dst, sport, dport, family}.
 * Device pointers; asynchronous on `stream`. */
NEB_API int neb_rx_coalesce_batch(neb_engine* e, const neb_plain_packet* d_plain, uint32_t n, const uint8_t* d_in,
                                  uint8_t* d_out, size_t out_cap, neb_tun_write* d_writes, uint32_t max_writes,
                                  uint32_t* d_nwrites, uint32_t* d_pkt_write, int32_t* d_pkt_status, uint32_t lanes,
                                  void* stream);
/* The same over host memory, on the CPU: the plain sequential algorithm, no engine and no GPU needed
 * (one routine's 64-packet flush). Every record is checked against in_len first (NEB_ERR_INVALID:
 * nothing written). */
NEB_API int neb_rx_coalesce_batch_host(const neb_plain_packet* plain, uint32_t n, const uint8_t* in, size_t in_len,
                                       uint8_t* out, size_t out_cap, neb_tun_write* writes, uint32_t max_writes,
                                       uint32_t* nwrites, uint32_t* pkt_write, int32_t* pkt_status, uint32_t lanes);
/* A finished neb_rx_open_wire_batch as commit records: packet i is committed iff status[i] ==
 * NEB_STATUS_OK, its header is type Message (1), subtype None (0) (outside.go:145-149) and key_id <
 * nepoch; then off = pk.off + 16, len = pk.len - 32, counter = header bytes 8:16, epoch =
 * epoch[key_id], flags 0 (the parse is derived). Every other packet gets NEB_PLAIN_SKIP. */
NEB_API int neb_rx_plain_from_wire(neb_engine* e, const neb_rx_packet* d_pk, const int32_t* d_status,
                                   const uint64_t* d_epoch, uint32_t nepoch, uint32_t n, const uint8_t* d_arena,
                                   neb_plain_packet* d_plain, void* stream);
NEB_API int neb_rx_plain_from_wire_host(const neb_rx_packet* pk, const int32_t* status, const uint64_t* epoch,
                                        uint32_t nepoch, uint32_t n, const uint8_t* arena, size_t arena_len,
                                        neb_plain_packet* plain);
/* ---- receive resolve: the hostmap's index lookups for a whole receive batch ---------------------- */
/* What readOutsidePackets looks up per datagram before it can decrypt: the tunnel of the header's
 * remote index (hostMap.QueryIndexCached / QueryRelayIndex, outside.go:93-100, hostmap.go:546-577),
 * the double-encryption check on the UDP source (f.myVpnNetworksTable.Contains, outside.go:66-74),
 * and, for Message/Relay, the relay's type and target (relayState.QueryRelayForByIdx,
 * QueryVpnAddrsRelayFor, outside.go:201-240). Each is a pure function of a 32-bit local index or of
 * an address over state that changes only at handshakes and relay set-up, so the state lives in a
 * table beside the keys and the windows, and one call fills neb_rx_packet.key_id,
 * NEB_RX_OWN_SOURCE, neb_relay_route and neb_rx_via for the calls above. */
#define NEB_INDEX_TUNNEL 0 /* hostMap.Indexes (hostmap.go:60, :669) */
#define NEB_INDEX_RELAY 1  /* hostMap.Relays  (hostmap.go:61) */
#define NEB_INDEX_MAX_NETWORKS 16
typedef struct neb_index_key {
    uint32_t index, space;
} neb_index_key;
typedef struct neb_index_entry {
    uint32_t index, space;
    uint32_t key_id;       /* the HostInfo's window / key slot; NEB_KEYS_MIXED: ConnectionState == nil */
    uint32_t flags;        /* relay space: NEB_VIA_TERMINAL for a TerminalType relay index */
    neb_relay_route route; /* relay space: the Established ForwardingType target, else {NEB_RELAY_NONE, 0} */
} neb_index_entry;
typedef struct neb_cidr { /* one of the node's own VPN networks (pki.go:477) */
    uint8_t addr[16];     /* family 4: the first 4 bytes */
    uint8_t family /* 4 | 6 */, bits, reserved[2];
} neb_cidr;
typedef struct neb_rx_source { /* the UDP source of a datagram, unmapped (udp/udp_linux.go:245) */
    uint8_t addr[16];          /* family 4: the first 4 bytes, the rest is ignored */
    uint8_t family /* 0 none, 4, 6 */, reserved[3];
} neb_rx_source;
typedef struct neb_index_table neb_index_table;

/* A table of at most `capacity` live entries (fixed; capacity >= 1). e == NULL: a host-only table
 * (neb_rx_resolve_batch_host only); otherwise the table also keeps its image in e's device memory. */
NEB_API int neb_index_table_create(neb_engine* e, uint32_t capacity, neb_index_table** out);
/* No call on the table may be in progress; waits for the device work the table has enqueued. */
NEB_API int neb_index_table_destroy(neb_index_table* t);
/* The deletions in array order, then the puts in array order. A put of a live key replaces its
 * record; deleting an absent key is not an error. NEB_ERR_INVALID (nothing applied): space > 1, or
 * a tunnel-space entry with flags != 0 or route.tunnel != NEB_RELAY_NONE. NEB_ERR_NO_KEY_SLOT
 * (nothing applied): more than `capacity` entries would be live after the call. Thread-safe.
 * Visibility of the device image: a resolve enqueued on `stream` after this call sees the update. A
 * resolve running on another stream meanwhile sees, for every key, its record from before or from
 * after this call, never a mix, and never a miss for a key that is live before and after. Updates
 * given on different streams take effect in the order of the calls. The call returns once its work
 * is enqueued, except when the table compacts itself (its deleted and replaced records have filled
 * 3/4 of its slots): it then waits for every resolve that still reads the spare image, writes that
 * image, waits for `stream`, and switches over, so it may block the calling control-plane thread
 * for as long as those batches take. stream is ignored by a host-only table. */
NEB_API int neb_index_table_update(neb_index_table* t, const neb_index_key* del, uint32_t ndel,
                                   const neb_index_entry* put, uint32_t nput, void* stream);
/* Replaces the node's own networks (at most NEB_INDEX_MAX_NETWORKS; NEB_ERR_INVALID: more, a family
 * other than 4 / 6, or bits beyond the family's width). Matching is netip.Prefix.Contains: a 4-byte
 * address against the v4 prefixes only, a 16-byte address, 4-in-6 included, against the v6 prefixes
 * only. Resolves called after this returns use the new set; stream is not used. */
NEB_API int neb_index_table_set_own_networks(neb_index_table* t, const neb_cidr* nets, uint32_t n, void* stream);
NEB_API int neb_index_table_count(const neb_index_table* t, uint32_t* live);
/* For tests, from the host copy: out = {found, slot, probes}: the slot of the key (found) or the
 * empty slot that ended the search, and the slots examined. */
NEB_API int neb_index_table_probe(const neb_index_table* t, uint32_t space, uint32_t index, uint32_t out[3]);
/* Per packet i, with len = pk[i].len without NEB_RX_OWN_SOURCE; off and len are the caller's:
 *   key = NEB_KEYS_MIXED, route = {NEB_RELAY_NONE, 0}, via = {NEB_KEYS_MIXED, 0};
 *   src given, src[i].family != 0 and the own networks contain src[i]: pk[i].len |= NEB_RX_OWN_SOURCE
 *   (the bit is never cleared);
 *   len >= 16: relay = (h[0] & 15) == 1 && h[1] == 1 for the header h at off, idx = BE32(h[4:8]);
 *   the entry of (relay ? NEB_INDEX_RELAY : NEB_INDEX_TUNNEL, idx), if any, gives key = key_id and,
 *   when relay: route = its route if route.tunnel != NEB_RELAY_NONE; if flags & NEB_VIA_TERMINAL,
 *   via.flags = NEB_VIA_TERMINAL and, when len >= 48, via.key_id = the key_id of the entry the
 *   header at off + 16 names the same way (its own relay bit chooses the space).
 * Every packet of 16 bytes or more is looked up, whatever its version and type: the drops and their
 * order stay with the receive calls' gate. Writes pk[i].key_id, the flag bit, route[i] and via[i]
 * (each array may be NULL: not written) and nothing else. n == 0 returns NEB_OK. The call only
 * enqueues one kernel on `stream`, in front of neb_rx_open_wire_batch / neb_relay_forward_batch /
 * neb_rx_open_via_batch on the same stream; d_src is 4-byte aligned. The caller reads pk[i].key_id
 * back together with status[i]. NEB_ERR_INVALID for a host-only table. */
NEB_API int neb_rx_resolve_batch(neb_engine* e, const neb_index_table* t, neb_rx_packet* d_pk,
                                 const neb_rx_source* d_src, uint32_t n, const uint8_t* d_arena,
                                 neb_relay_route* d_route, neb_rx_via* d_via, void* stream);
/* The same over host memory, from the table's host copy (any table). Every pk is checked against
 * arena_len first (NEB_ERR_INVALID: nothing written). */
NEB_API int neb_rx_resolve_batch_host(const neb_index_table* t, neb_rx_packet* pk, const neb_rx_source* src,
                                      uint32_t n, const uint8_t* arena, size_t arena_len, neb_relay_route* route,
                                      neb_rx_via* via);
/* ---- RX receive plan: UDP_GRO receive entries -> wire packets ----------------------------------- */
/* What StdConn.ListenOut does with a recvmmsg batch before readOutsidePackets sees a packet
 * (udp/udp_linux.go:274-284): with UDP_GRO on (udp_linux.go:78-108) one entry is a superdatagram, a
 * gso_size in a control message and a raw sockaddr, and getFrom (:237-246), parseRecvCmsg (:307-331)
 * and deliverSegments (:291-303) turn it into wire packets. The call does that for a whole batch and
 * writes the neb_rx_packet / neb_rx_source arrays neb_rx_resolve_batch takes. The plan only names
 * bytes: it never reads the arena. */
#define NEB_RECV_NONE 0xFFFFFFFFu
typedef struct neb_recv_entry {   /* one recvmmsg slot after the call; 48 bytes, 8-byte aligned */
    uint64_t off;                 /* the slot's buffer in the arena */
    uint32_t len;                 /* mmsghdr.msg_len */
    int32_t  seg_size;            /* the UDP_GRO size when the caller parsed it (d_ctrl == NULL) */
    uint8_t  name[28];            /* msg_name as the kernel wrote it (sockaddr_in / sockaddr_in6) */
    uint32_t ctrl_len;            /* msg_controllen after the call (d_ctrl != NULL) */
} neb_recv_entry;
/* Per entry j, in entry order:
 *   its segment size is entries[j].seg_size when d_ctrl == NULL; otherwise parseRecvCmsg over the L =
 *   min(ctrl_len, ctrl_stride) bytes at d_ctrl + j * ctrl_stride, and no byte at or past L is read.
 *   Linux LP64, little-endian: cmsghdr = {u64 len; i32 level; i32 type}, SizeofCmsghdr = CmsgLen(0) =
 *   16, CmsgSpace(n) = 16 + align8(n). The walk starts at 0 with size 0 and is the reference's, hostile
 *   input included: it stops when off + 16 > L; it returns what it has when len < 16 or len > L - off
 *   (len as the reference's signed int, so 2^63 is negative); at level SOL_UDP (17), type UDP_GRO (104),
 *   if off + 16 + 4 <= L the size is the int32 at off + 16, and the last match wins; it advances by
 *   align8(len);
 *   its packets are deliverSegments': size <= 0 or size >= len gives one packet {off, len} (len == 0
 *   too: one empty packet); otherwise ceil(len / size) packets, packet k = {off + k * size, min(size,
 *   len - k * size)}, offsets in 64 bits. Every entry yields at least one packet;
 *   its source is getFrom's: the port is big-endian at name[2:4]; the address is name[4:8] when
 *   socket_v4 != 0, else name[8:24], unmapped: an address in ::ffff:0:0/96 becomes family 4 with its
 *   last four bytes. The sockaddr's family field and its other bytes are ignored, as there.
 * Packets are numbered in entry order: first[j] is the sum of the counts before j, carried in 64 bits
 * (one entry may hold 2^32 - 1 one-byte packets). Entry j is emitted iff first[j] + count[j] <=
 * max_packets, so the emitted entries are a prefix: counts[1] = nentries_done is its length and
 * counts[0] = npackets its packets. An emitted entry has entry_first[j] = first[j]; every other one
 * has NEB_RECV_NONE and emits nothing: the caller plans it again with its next batch.
 * Per emitted packet i of entry j: pk[i] = {off, len, NEB_KEYS_MIXED} (NEB_RX_OWN_SOURCE is never
 * set: the resolve does that), pkt_entry[i] = j, src[i] = the source as neb_rx_resolve_batch wants it
 * (for family 4 the address's other 12 bytes zero, reserved zero). Per entry j < nentries, emitted or
 * not: from[j] = the source with its port (family 4 or 6, unused address bytes and reserved zero),
 * for a later roaming check, which needs the port.
 * Slots i in [npackets, max_packets) are written as padding: pk[i] = {0, 0, NEB_KEYS_MIXED},
 * src[i] all zero (family 0), pkt_entry[i] = NEB_RECV_NONE. Unlike the send plan: neb_rx_resolve_batch
 * and neb_rx_open_wire_batch take n by value, so a caller runs them over max_packets on the same
 * stream with no read-back; their gate gives padding NEB_STATUS_INVALID and touches nothing. The
 * call's cost follows nentries + max_packets. pk, src and pkt_entry hold max_packets elements, from
 * and entry_first nentries, counts two; nothing beyond is written. src, pkt_entry and from may be
 * NULL: not written.
 * nentries == 0: counts = {0, 0}, every slot padding. max_packets == 0: counts = {0, 0}, every entry
 * NEB_RECV_NONE.
 * Device pointers (d_entries and d_ctrl 8-byte, the others 4-byte aligned); asynchronous on `stream`,
 * no read-back, no synchronisation, so neb_rx_resolve_batch and the receive calls follow it on its
 * stream directly.
 * NEB_ERR_INVALID: e, d_pk, d_entry_first or d_counts NULL; d_entries NULL with nentries != 0;
 * nentries or max_packets >= 2^31; d_ctrl given with a ctrl_stride of 0, not a multiple of 8, or
 * above 1024; d_entries or d_ctrl not 8-byte aligned.
 * Not part of the plan: the socket, recvmmsg, and handleHostRoaming (outside.go), whose allow-list
 * and time-based suppression are control plane; from[] and pkt_entry[] are what it reads, reduced to
 * one record per run by neb_rx_report_batch. */
NEB_API int neb_rx_recv_plan(neb_engine* e, const neb_recv_entry* d_entries, uint32_t nentries,
                             const uint8_t* d_ctrl /* may be NULL */, uint32_t ctrl_stride, uint32_t socket_v4,
                             neb_rx_packet* d_pk, neb_rx_source* d_src /* may be NULL */,
                             uint32_t* d_pkt_entry /* may be NULL */, uint32_t max_packets,
                             neb_udp_addr* d_from /* may be NULL */, uint32_t* d_entry_first,
                             uint32_t* d_counts /* {npackets, nentries_done} */, void* stream);
/* The same over host memory: the plain sequential loop, no engine, no GPU. */
NEB_API int neb_rx_recv_plan_host(const neb_recv_entry* entries, uint32_t nentries,
                                  const uint8_t* ctrl /* may be NULL */, uint32_t ctrl_stride, uint32_t socket_v4,
                                  neb_rx_packet* pk, neb_rx_source* src /* may be NULL */,
                                  uint32_t* pkt_entry /* may be NULL */, uint32_t max_packets,
                                  neb_udp_addr* from /* may be NULL */, uint32_t* entry_first,
                                  uint32_t* counts /* {npackets, nentries_done} */);
/* ---- RX batch report: roaming runs, traffic marks, metrics, host work list ----------------------- */
/* The side effects of readOutsidePackets (outside.go:30-189) and handleOutsideRelayPacket (:191-200)
 * that are not the packet's bytes: messageMetrics.Rx / RxInvalid (message_metrics.go),
 * handleHostRoaming, connectionManager.In / RelayUsed, the dispatch of the control types and
 * maybeSendRecvError. One call behind neb_rx_open_wire_batch reduces a batch's statuses, headers,
 * tunnels and sources to what the control plane acts on, so the caller loops over tunnels, not packets
 * (DESIGN.md §3.17). */
#define NEB_REPORT_RELAYED 1u   /* the packets came out of terminal relay packets (IsRelayed) */
#define NEB_REPORT_NMETRICS 16
#define NEB_METRIC_RX_HANDSHAKE 0      /* messages.rx.handshake_ixpsk0 */
#define NEB_METRIC_RX_RECV_ERROR 1     /* messages.rx.recv_error */
#define NEB_METRIC_RX_LIGHTHOUSE 2     /* messages.rx.lighthouse */
#define NEB_METRIC_RX_TEST_REQUEST 3   /* messages.rx.test_request */
#define NEB_METRIC_RX_TEST_RESPONSE 4  /* messages.rx.test_response */
#define NEB_METRIC_RX_CLOSE_TUNNEL 5   /* messages.rx.close_tunnel */
#define NEB_METRIC_RX_OTHER 6          /* messages.rx.other: Control, which newMessageMetrics gives no row */
#define NEB_METRIC_RX_INVALID 7        /* messages.rx.invalid */
#define NEB_METRIC_OPENED 8            /* packets with NEB_STATUS_OK */
#define NEB_METRIC_OPENED_BYTES 9      /* ... and the sum of their wire lengths */
#define NEB_METRIC_AUTH_FAILED 10      /* NEB_STATUS_AUTH_FAILED */
#define NEB_METRIC_REPLAY 11           /* NEB_STATUS_REPLAY */
#define NEB_METRIC_NO_TUNNEL 12        /* NEB_STATUS_BAD_KEY with key_id == NEB_KEYS_MIXED; 13..15: written as 0 */
#define NEB_WORK_HANDSHAKE 1       /* handshakeManager.HandleIncoming (outside.go:84) */
#define NEB_WORK_RECV_ERROR 2      /* handleRecvError (:88) */
#define NEB_WORK_NESTED_RELAY 3    /* a Message/Relay inside a relay: one more level, the caller's */
#define NEB_WORK_SEND_RECV_ERROR 4 /* maybeSendRecvError (:106): endpoint from from[], index from the header */
#define NEB_WORK_LIGHTHOUSE 5      /* lhh.HandleRequest (:157) */
#define NEB_WORK_TEST_REQUEST 6    /* the Test reply (:163-173) */
#define NEB_WORK_CLOSE_TUNNEL 7    /* closeTunnel (:181) */
#define NEB_WORK_CONTROL 8         /* relayManager.HandleControlMsg (:184) */
typedef struct neb_rx_run {     /* consecutive authenticated packets of one tunnel from one source; 40 bytes */
    uint64_t bytes;             /* sum of their wire lengths */
    uint32_t key_id, packet /* the first one's index */, packets;
    neb_udp_addr from;          /* all zero (family 0) when the packet has no source */
} neb_rx_run;
typedef struct neb_rx_relay_used { uint32_t index, packets; } neb_rx_relay_used;
typedef struct neb_rx_work { uint32_t packet, kind; } neb_rx_work; /* kind: NEB_WORK_* */
/* Per packet i < n: len is pk[i].len without NEB_RX_OWN_SOURCE; h, the 16 bytes at pk[i].off, is read
 * only when len >= 16 (the header of an opened packet is intact: the open is in place behind it).
 *   Source: from[pkt_entry[i]] with d_pkt_entry (the receive plan's outputs), else from[i]; all zero
 *   when d_from is NULL, NEB_REPORT_RELAYED is set, or the index is NEB_RECV_NONE or >= nfrom (the
 *   receive plan's padding never indexes from[]).
 *   Metrics, in the gate's order (outside.go:32-79): rx.invalid counts status == NEB_STATUS_INVALID
 *   with len > 1 (hole punches and padding are not counted). A packet with len >= 16, version 1, a
 *   valid subtype and no NEB_RX_OWN_SOURCE (ignored with NEB_REPORT_RELAYED) counts Rx(type, subtype)
 *   when its type is not Message, whatever its status ends as: no tunnel, len < 32, a failed tag, a
 *   replay. Slots: NEB_METRIC_*; 13..15 are written as 0.
 *   Authenticated: status == NEB_STATUS_OK (replays and failed tags return before outside.go:142).
 *   These packets, and only these, enter runs and relay_used.
 *   Runs: the authenticated packets sorted by (key_id, packet index); a run starts where key_id
 *   changes or the 20-byte source differs from the previous packet's of that tunnel; runs are emitted
 *   in that order, a tunnel's first run always (no remote[] snapshot is taken). counts[1] = ntunnels
 *   is the number of distinct key_ids. The caller does connectionManager.In once per distinct key_id
 *   and the unchanged handleHostRoaming(hostinfo, run.from) once per run whose from.family is not 0.
 *   Leaving a repeat of the previous source out is exact: the second call with the same via is a
 *   no-op or refused as the first was (DESIGN.md §3.17 names the one exception, a suppression that
 *   expires between two packets of one batch).
 *   relay_used: the distinct BE32(h[4:8]) of authenticated Message/Relay packets, ascending, each with
 *   its packet count, for connectionManager.RelayUsed.
 *   Work list, in arrival order: NEB_STATUS_NOT_MESSAGE gives HANDSHAKE (type 0), RECV_ERROR (type 2)
 *   or, with NEB_REPORT_RELAYED, NESTED_RELAY (Message/Relay); NEB_STATUS_BAD_KEY with key_id ==
 *   NEB_KEYS_MIXED and not relayed gives SEND_RECV_ERROR; NEB_STATUS_OK with type 3, 4/0, 5 or 6 gives
 *   LIGHTHOUSE, TEST_REQUEST, CLOSE_TUNNEL or CONTROL. TestReply is a no-op there and is not listed.
 *   A packet shorter than 16 bytes is never listed.
 * Every output array holds n elements; runs, relay_used and work are written up to their counts and
 * nothing beyond. n == 0: counts and metrics zeroed.
 * Device pointers (d_runs and d_metrics 8-byte, the others 4-byte aligned); asynchronous on `stream`,
 * no read-back, no synchronisation: it follows neb_rx_open_wire_batch on its stream directly. For a
 * via batch it is called twice: for the outer packets, and for inner_pk / inner_status with
 * NEB_REPORT_RELAYED.
 * NEB_ERR_INVALID: e, d_counts or d_metrics NULL; with n != 0, d_pk, d_status, d_arena, d_runs,
 * d_relay_used or d_work NULL; n >= 2^31; a misaligned pointer; an unknown bit in flags.
 * Not part of the report: neb_relay_forward_batch rewrites the outer header of forwarded packets in
 * place, so their original relay index is gone by the time statuses exist and RelayUsed for forwarded
 * packets stays with the caller (runs and metrics remain valid for that call); handleHostRoaming's
 * allow list and timers, and the connection manager itself; a CloseTunnel that takes effect on later
 * packets of its own batch (table updates apply between batches); the TX side (connectionManager.Out). */
NEB_API int neb_rx_report_batch(neb_engine* e, const neb_rx_packet* d_pk, const int32_t* d_status, uint32_t n,
                                const uint8_t* d_arena, const neb_udp_addr* d_from /* may be NULL */,
                                const uint32_t* d_pkt_entry /* may be NULL: d_from is per packet */, uint32_t nfrom,
                                uint32_t flags, neb_rx_run* d_runs, neb_rx_relay_used* d_relay_used, neb_rx_work* d_work,
                                uint64_t* d_metrics /* [NEB_REPORT_NMETRICS] */,
                                uint32_t* d_counts /* {nruns, ntunnels, nrelay_used, nwork} */, void* stream);
/* The same over host memory: the plain sequential loop, no engine, no GPU. Every packet of 16 bytes
 * or more is checked against arena_len first (NEB_ERR_INVALID: nothing written). */
NEB_API int neb_rx_report_batch_host(const neb_rx_packet* pk, const int32_t* status, uint32_t n, const uint8_t* arena,
                                     size_t arena_len, const neb_udp_addr* from /* may be NULL */,
                                     const uint32_t* pkt_entry /* may be NULL */, uint32_t nfrom, uint32_t flags,
                                     neb_rx_run* runs, neb_rx_relay_used* relay_used, neb_rx_work* work,
                                     uint64_t* metrics, uint32_t* counts);
/* ---- TX resolve: parse, own-address gates and VPN address / route lookup for a TX batch -------- */
/* The front half of consumeInsidePacket (inside.go:19-121) for a whole batch of TUN reads: newPacket
 * (outside.go:320-472, iputil/packet.go:349-395), the local-broadcast, self and multicast gates
 * (inside.go:43-76) and getOrHandshakeConsiderRouting (inside.go:292-372): Hosts[vpnAddr], the
 * longest-prefix match over the unsafe routes (overlay/tun_linux.go:366-369) and ECMP
 * (routing/balance.go, routing/gateway.go:57-70). Each is a pure function of the packet's first
 * bytes over state that changes only at handshakes and config reloads, so the state lives in a table
 * beside the tunnel array and one call fills neb_tx_packet.tunnel for neb_tx_seal_batch /
 * neb_tx_seal_via_batch, and hands the caller's firewall its input (firewall.Packet). */
#define NEB_STATUS_TX_DROPPED 10 /* a gate dropped the read (which one: neb_fw_packet.flags) */
#define NEB_STATUS_NO_ROUTE 11   /* not in an own network and no route covers it (rejectInside) */
#define NEB_STATUS_NO_TUNNEL 12  /* no host entry yet: the caller handshakes */
#define NEB_TX_NO_TUNNEL 0xFFFFFFFFu /* neb_tx_packet.tunnel of a read that is not to be sealed */
#define NEB_GATEWAY_NONE 0xFFFFFFFFu
#define NEB_ROUTE_MAX_GATEWAYS 16
#define NEB_TX_DROP_LOCAL_BROADCAST 1u /* f.dropLocalBroadcast */
#define NEB_TX_DROP_MULTICAST 2u       /* f.dropMulticast */
#define NEB_TX_KIND_HOST 0
#define NEB_TX_KIND_ROUTE 1
#define NEB_FW_FRAGMENT 0x01       /* ParsedPacket.Fragment: a non-first fragment, ports are 0 */
#define NEB_FW_FRAG_ANY 0x02       /* ParsedPacket.FragAny: MF or an offset (v6: a fragment header) */
#define NEB_FW_GATE_BROADCAST 0x04 /* dropped: an own IPv4 network's broadcast address */
#define NEB_FW_GATE_SELF 0x08      /* dropped: one of the own VPN addresses */
#define NEB_FW_GATE_MULTICAST 0x10 /* dropped: multicast */
#define NEB_FW_ROUTED 0x20         /* a route was used: the tunnel is a gateway's */
#define NEB_FW_ECMP_FALLBACK 0x40  /* the gateway ECMP chose has no tunnel; another one's was taken */
typedef struct neb_tx_addr { /* a VPN address */
    uint8_t addr[16];        /* family 4: the first 4 bytes, the rest is ignored */
    uint8_t family /* 4 | 6; a 4-in-6 address is family 6 and never equals its IPv4 form */, reserved[3];
} neb_tx_addr;
typedef struct neb_tx_host { /* hostMap.Hosts[vpnAddr] (hostmap.go) */
    neb_tx_addr addr;
    uint32_t tunnel; /* index into the caller's neb_tx_tunnel array */
} neb_tx_host;
typedef struct neb_gateway { /* routing.Gateway */
    neb_tx_addr addr;
    uint32_t weight; /* used on a route of several gateways only */
} neb_gateway;
typedef struct neb_route { /* one unsafe route; the prefix's host bits are ignored, as bart's Insert does */
    neb_cidr prefix;
    uint32_t ngateways; /* 1..NEB_ROUTE_MAX_GATEWAYS */
    neb_gateway gateways[NEB_ROUTE_MAX_GATEWAYS];
} neb_route;
/* firewall.ParsedPacket of an outgoing packet, and how the lookup went. 16-byte aligned. */
typedef struct neb_fw_packet {
    uint8_t local_addr[16];  /* family 4: the first 4 bytes, the rest 0 */
    uint8_t remote_addr[16];
    uint16_t local_port, remote_port; /* host order; ICMP / ICMPv6 echo: remote_port = identifier */
    uint8_t protocol;
    uint8_t family; /* 4 | 6 */
    uint8_t flags;  /* NEB_FW_* */
    uint8_t reserved;
    uint16_t ip_hdr_len; /* ParsedPacket.IPHdrLen: where the upper protocol starts */
    uint16_t reserved2;
    uint32_t gateway; /* flat index, in neb_tx_table_set_routes order, of the gateway ECMP chose or of
                         the single gateway; NEB_GATEWAY_NONE when no route was used */
} neb_fw_packet;
typedef struct neb_tx_table neb_tx_table;

/* A table of at most host_capacity host entries, route_capacity routes and gateway_capacity
 * gateways over all routes (fixed; host_capacity >= 1; each at most 2^20: NEB_ERR_INVALID beyond, and
 * when the host copy, 128 to 256 bytes per host and route, cannot be allocated). e == NULL: a host-only
 * table (neb_tx_resolve_batch_host only); otherwise the table also keeps its images in e's device
 * memory. */
NEB_API int neb_tx_table_create(neb_engine* e, uint32_t host_capacity, uint32_t route_capacity,
                                uint32_t gateway_capacity, neb_tx_table** out);
/* No call on the table may be in progress; waits for the device work the table has enqueued. */
NEB_API int neb_tx_table_destroy(neb_tx_table* t);
/* Host entries change with every handshake. The deletions in array order, then the puts in array
 * order; a put of a live address replaces its tunnel; deleting an absent address is not an error.
 * NEB_ERR_INVALID (nothing applied): a family other than 4 / 6, or the call's own bookkeeping
 * could not be allocated. NEB_ERR_NO_KEY_SLOT (nothing
 * applied): more than host_capacity entries would be live after the call. Thread-safe. Visibility
 * is neb_index_table_update's: a resolve enqueued on `stream` after this call sees the update; a
 * resolve running on another stream meanwhile sees, for every address, its tunnel from before or
 * from after this call, never a mix, and never a miss for an address that is live before and after.
 * Updates given on different streams take effect in the order of the calls. The call returns once
 * its work is enqueued, except when the table compacts itself (deleted and replaced records have
 * filled 3/4 of its slots): it then waits for every resolve that still reads the spare image, writes
 * that image, waits for `stream`, and switches over. Meanwhile other updates, neb_tx_table_set_own
 * and neb_tx_resolve_batch_host on this table wait for the call; neb_tx_resolve_batch does not: it
 * goes on enqueueing resolves of the image that is still active. stream is ignored by a host-only
 * table. */
NEB_API int neb_tx_table_update_hosts(neb_tx_table* t, const neb_tx_addr* del, uint32_t ndel,
                                      const neb_tx_host* put, uint32_t nput, void* stream);
/* Routes change at a config reload only. Replaces the whole route set (nroutes == 0: none) through
 * the compaction path above, so the call always blocks the calling thread until the spare image is
 * written and switched to (who else waits meanwhile: as for a compaction above): every resolve sees
 * one route set in its entirety, the new one if it was enqueued after the call returned, the old
 * or the new one if it was enqueued while the call ran. A route of several gateways gets its ECMP
 * buckets here (CalculateBucketsForGateways, routing/gateway.go:57-70). A gateway's tunnel is its
 * host entry at resolve time, so a gateway's tunnel coming or going needs no route update.
 * NEB_ERR_INVALID (nothing applied): ngateways == 0 or > NEB_ROUTE_MAX_GATEWAYS, a total weight of 0
 * on a route of several gateways (the reference would divide by zero), a bad family or prefix
 * length, two routes with the same masked prefix, or no memory for the new set. NEB_ERR_NO_KEY_SLOT (nothing applied): more
 * than route_capacity routes or gateway_capacity gateways. */
NEB_API int neb_tx_table_set_routes(neb_tx_table* t, const neb_route* routes, uint32_t nroutes, void* stream);
/* The node's own networks (at most NEB_INDEX_MAX_NETWORKS), `addr` holding the node's own address in
 * the network, unmasked (pki.go:475-487): gives the prefixes (myVpnNetworksTable), the own
 * addresses (myVpnAddrsTable) and the IPv4 broadcast addresses network | ~mask
 * (myVpnBroadcastAddrsTable). flags: NEB_TX_DROP_*. NEB_ERR_INVALID: more networks, a bad family or
 * prefix length, unknown flags. Resolves called after this returns use the new set. */
NEB_API int neb_tx_table_set_own(neb_tx_table* t, const neb_cidr* nets, uint32_t n, uint32_t flags);
NEB_API int neb_tx_table_count(const neb_tx_table* t, uint32_t* hosts, uint32_t* routes);
/* For tests, from the host copy: kind NEB_TX_KIND_HOST (key->bits ignored) or NEB_TX_KIND_ROUTE (the
 * prefix is masked first); out = {found, slot, probes} as neb_index_table_probe. */
NEB_API int neb_tx_table_probe(const neb_tx_table* t, uint32_t kind, const neb_cidr* key, uint32_t out[3]);
/* Per TUN read i, the IP packet of packets[i].len bytes at packets[i].in_off (no alignment; nothing
 * beyond those bytes is read):
 *   newPacket(pkt, false, fp) fails: status NEB_STATUS_INVALID; fw[i] is zero but for ip_hdr_len and
 *   NEB_FW_FRAG_ANY as newPacket had left them. Otherwise fw[i] is the ParsedPacket and
 *   drop_local_broadcast and the remote address is an own IPv4 network's broadcast address, or
 *   the remote address is an own address, or
 *   drop_multicast and it is multicast (224.0.0.0/4, ff00::/8, a 4-in-6 address unmapped first, as
 *   netip's IsMulticast does): NEB_STATUS_TX_DROPPED with that gate's NEB_FW_GATE_* flag;
 *   the remote address is in an own network (netip.Prefix.Contains): its host entry gives the tunnel,
 *   none is NEB_STATUS_NO_TUNNEL (routes are not consulted);
 *   otherwise the longest route prefix containing it: none is NEB_STATUS_NO_ROUTE; else
 *   NEB_FW_ROUTED, and with one gateway fw.gateway is that gateway; with several, h = hashPacket(
 *   local_port, remote_port) and fw.gateway is the first with h <= its bucket's upper bound. Its
 *   host entry gives the tunnel; without one, on a route of several gateways, the first gateway in
 *   list order with another address and a host entry gives it (NEB_FW_ECMP_FALLBACK; fw.gateway
 *   stays the chosen one); else NEB_STATUS_NO_TUNNEL.
 * packets[i].tunnel is always written: the tunnel on NEB_STATUS_OK, else NEB_TX_NO_TUNNEL, which a
 * following neb_tx_seal_batch / neb_tx_seal_via_batch on the same stream answers with
 * NEB_STATUS_BAD_KEY, no wire and no counter. On NEB_STATUS_NO_TUNNEL the caller handshakes with
 * remote_addr when fw.gateway is NEB_GATEWAY_NONE, else with that gateway's address. d_fw (16-byte
 * aligned) and d_status may be NULL: not written. Only enqueues one kernel on `stream`.
 * NEB_ERR_INVALID for a host-only table. */
NEB_API int neb_tx_resolve_batch(neb_engine* e, const neb_tx_table* t, neb_tx_packet* d_packets, uint32_t npackets,
                                 const uint8_t* d_in, neb_fw_packet* d_fw, int32_t* d_status, void* stream);
/* The same over host memory, from the table's host copy (any table). Every packet is checked
 * against in_len first (NEB_ERR_INVALID: nothing written). */
NEB_API int neb_tx_resolve_batch_host(const neb_tx_table* t, neb_tx_packet* packets, uint32_t npackets,
                                      const uint8_t* in, size_t in_len, neb_fw_packet* fw, int32_t* status);
/* ---- RX inner resolve: parse opened packets, check the peer's and the own addresses ------------- */
/* What handleOutsideMessagePacket does between Decrypt and Commit (outside.go:474-494) short of the
 * rules and conntrack: newPacket(out, true, fwPacket) and the first two checks of firewall.Drop
 * (firewall.go:425-457): the inner source address must belong to the peer's certificate
 * (h.networks.Lookup(fp.RemoteAddr), hostmap.go:837-857) and the inner destination to our routable
 * networks (routableNetworks.Contains(fp.LocalAddr), firewall.go:154-165). Both are pure functions of
 * the packet's first bytes over state that changes only at handshakes and config reloads, so the state
 * lives in a table beside the keys, and one call takes neb_rx_plain_from_wire's place between
 * neb_rx_open_wire_batch / neb_rx_open_via_batch and neb_rx_coalesce_batch. */
#define NEB_STATUS_RX_BAD_REMOTE 13    /* ErrInvalidRemoteIP */
#define NEB_STATUS_RX_PEER_REJECTED 14 /* ErrPeerRejected */
#define NEB_STATUS_RX_BAD_LOCAL 15     /* ErrInvalidLocalIP */
#define NEB_NET_VPN 1      /* NetworkTypeVPN (hostmap.go:228-238) */
#define NEB_NET_VPN_PEER 2 /* NetworkTypeVPNPeer */
#define NEB_NET_UNSAFE 3   /* NetworkTypeUnsafe */
#define NEB_RX_MAX_ROUTABLE 32
typedef struct neb_peer_net { /* one entry of a HostInfo's networks table */
    uint32_t tunnel;          /* the packets' key_id: the window / key slot; never NEB_KEYS_MIXED */
    uint32_t type;            /* NEB_NET_* */
    neb_cidr prefix;          /* host bits are ignored, as bart's Insert does */
} neb_peer_net;
typedef struct neb_peer_key {
    uint32_t tunnel;
    neb_cidr prefix;
} neb_peer_key;
typedef struct neb_peer_table neb_peer_table;

/* A table of at most `capacity` live entries over all tunnels (fixed; 1..2^20). e == NULL: a
 * host-only table (neb_rx_inner_batch_host only); otherwise the table also keeps its image in e's
 * device memory. An entry's key is (tunnel, family, bits, masked prefix). The simple case of
 * firewall.Drop (h.networks == nil: the remote address must equal h.vpnAddrs[0]) has no form of its
 * own: it is a tunnel with one full-length NEB_NET_VPN entry. */
NEB_API int neb_peer_table_create(neb_engine* e, uint32_t capacity, neb_peer_table** out);
/* No call on the table may be in progress; waits for the device work the table has enqueued. */
NEB_API int neb_peer_table_destroy(neb_peer_table* t);
/* A tunnel's entries come with its handshake and go when it closes. The deletions in array order,
 * then the puts in array order; a put of a live key replaces its type (so puts in buildNetworks'
 * order give the reference's overwrite when an unsafe network equals a VPN address); deleting an
 * absent key is not an error. NEB_ERR_INVALID (nothing applied): a type outside 1..3, a bad family
 * or prefix length, tunnel == NEB_KEYS_MIXED, or the call's bookkeeping could not be allocated.
 * NEB_ERR_NO_KEY_SLOT (nothing applied): more than `capacity` entries would be live after the call.
 * Thread-safe. Visibility, ordering and compaction are neb_tx_table_update_hosts': a call enqueued on
 * `stream` after this one sees the update; one running on another stream meanwhile sees, for every
 * key, its record from before or from after, and never misses a key that is live before and after;
 * when deleted and replaced records have filled 3/4 of the slots the call rebuilds the spare image
 * and blocks until it has switched over. stream is ignored by a host-only table. */
NEB_API int neb_peer_table_update(neb_peer_table* t, const neb_peer_key* del, uint32_t ndel, const neb_peer_net* put,
                                  uint32_t nput, void* stream);
/* Replaces the routable set (firewall.go:154-165): the own VPN addresses at full length and the own
 * unsafe networks, at most NEB_RX_MAX_ROUTABLE (NEB_ERR_INVALID: more, a bad family or prefix
 * length). Calls made after this returns use the new set. */
NEB_API int neb_peer_table_set_routable(neb_peer_table* t, const neb_cidr* nets, uint32_t n);
NEB_API int neb_peer_table_count(const neb_peer_table* t, uint32_t* live);
/* For tests, from the host copy: out = {found, slot, probes} as neb_index_table_probe. */
NEB_API int neb_peer_table_probe(const neb_peer_table* t, const neb_peer_key* key, uint32_t out[3]);
/* pk / status: a finished neb_rx_open_wire_batch, or the inner_pk / inner_status of
 * neb_rx_open_via_batch. Per packet i, with len = pk[i].len without NEB_RX_OWN_SOURCE:
 *   not committed by neb_rx_plain_from_wire's rule (status OK, header Message / None, key_id < nepoch,
 *   len >= 32): plain[i] as that call writes it (NEB_PLAIN_SKIP), fw[i] zero, inner status
 *   NEB_STATUS_NOT_MESSAGE;
 *   newPacket(data, true, fp) over the len - 32 bytes at off + 16 fails: NEB_STATUS_INVALID, plain[i]
 *   as above, fw[i] zero but for ip_hdr_len and NEB_FW_FRAG_ANY as newPacket had left them;
 *   otherwise fw[i] is the ParsedPacket, locally oriented (remote = the inner source; the ICMP /
 *   ICMPv6-echo identifier is remote_port, local_port 0), gateway NEB_GATEWAY_NONE, and
 *   the longest prefix among tunnel key_id's entries that contains the remote address (netip's
 *   families: a 4-byte address matches v4 entries only, a 16-byte one, 4-in-6 included, v6 entries
 *   only): none is NEB_STATUS_RX_BAD_REMOTE, NEB_NET_VPN_PEER is NEB_STATUS_RX_PEER_REJECTED;
 *   then the routable set does not contain the local address: NEB_STATUS_RX_BAD_LOCAL;
 *   a refused packet gets NEB_PLAIN_SKIP in plain[i] (fw[i] stays the parse: the caller's
 *   rejectOutside); a passing one NEB_STATUS_OK and neb_rx_plain_from_wire's record with
 *   NEB_PLAIN_PARSED, proto, ip_hdr_len and NEB_PLAIN_FRAG_ANY, which neb_rx_coalesce_batch then uses
 *   instead of deriving them.
 * Writes plain, fw and inner_status (the last two may be NULL: not written) and nothing else; reads
 * the 16-byte header and [off + 16, off + len - 16) of a packet and nothing else of the arena.
 * d_plain and d_fw are 16-byte aligned. n == 0 returns NEB_OK. Only enqueues one kernel on `stream`.
 * NEB_ERR_INVALID for a host-only table. */
NEB_API int neb_rx_inner_batch(neb_engine* e, const neb_peer_table* t, const neb_rx_packet* d_pk,
                               const int32_t* d_status, const uint64_t* d_epoch, uint32_t nepoch, uint32_t n,
                               const uint8_t* d_arena, neb_plain_packet* d_plain, neb_fw_packet* d_fw,
                               int32_t* d_inner_status, void* stream);
/* The same over host memory, from the table's host copy (any table). Every pk is checked against
 * arena_len first (NEB_ERR_INVALID: nothing written). */
NEB_API int neb_rx_inner_batch_host(const neb_peer_table* t, const neb_rx_packet* pk, const int32_t* status,
                                    const uint64_t* epoch, uint32_t nepoch, uint32_t n, const uint8_t* arena,
                                    size_t arena_len, neb_plain_packet* plain, neb_fw_packet* fw,
                                    int32_t* inner_status);
/* ---- conntrack: firewall.Conntrack.Conns for TX and RX batches --------------------------------- */
/* firewall.Drop asks inConns before it looks at any rule (firewall.go:459-478), and an established
 * flow never reaches the rules. The map[firewall.Packet]*conn lives in a table beside the others and
 * answers the three operations the reference does on it: inConns (lookup), addConn (add) and evict
 * (firewall.go:505-630). Rule evaluation and the timer wheel stay with the caller: after a lookup
 * only the packets of new flows and of flows added under older rules leave the device, as a compact
 * work list; established flows go straight on to neb_rx_coalesce_batch or neb_tx_seal_batch.
 * The key is LocalAddr, RemoteAddr, LocalPort, RemotePort, Protocol and Fragment, taken from a
 * neb_fw_packet: local_addr, remote_addr, local_port, remote_port, protocol, family and the
 * NEB_FW_FRAGMENT bit of flags. For family 4 only the first 4 address bytes count (bytes 4..15 of the
 * input are not trusted); a 4-in-6 address never equals its IPv4 form, as with netip. ip_hdr_len,
 * gateway, the other flag bits and the reserved fields are not part of the key. The value is Expires
 * (ns of the caller's monotonic clock), incoming and rulesVersion.
 * Concurrency: add, evict, compact and set_rules_version on one table are serialised by the caller
 * (one stream, or waits); lookups may run on any stream at the same time as an add or an evict, and a
 * key that stays in the table never misses. Nothing may run during neb_conntrack_compact. */
#define NEB_STATUS_FW_HELD 18 /* the conntrack lookup held the packet for the caller's rules */
#define NEB_CT_NONE 0         /* verdict: input status != NEB_STATUS_OK, not looked up */
#define NEB_CT_HIT 1          /* established: Expires refreshed */
#define NEB_CT_MISS 2         /* no entry: the caller's rules decide */
#define NEB_CT_STALE 3        /* an entry of another rulesVersion, untouched (firewall.go:527-560) */
#define NEB_CT_INCOMING 0x80  /* or-ed into a STALE verdict: the entry's incoming */
#define NEB_CT_NEW 1          /* add: inserted; the caller adds the key to its timer wheel */
#define NEB_CT_EXISTING 2     /* add: the entry's three fields overwritten; no wheel add */
#define NEB_CT_DUP 3          /* add: another copy of the key in this batch answered NEW or EXISTING */
#define NEB_CT_FULL 4         /* add: refused, nothing changed; slot is NEB_CT_NO_SLOT */
#define NEB_CT_NO_SLOT 0xFFFFFFFFu
typedef struct neb_ct_work { /* one packet for the caller's rules. 16-byte aligned. */
    uint32_t packet;         /* index in the batch */
    uint32_t verdict;        /* NEB_CT_MISS, or NEB_CT_STALE [| NEB_CT_INCOMING] */
    neb_fw_packet fw;        /* the packet's input record, as given */
    uint8_t reserved[8];     /* 0 */
} neb_ct_work;
typedef struct neb_ct_result {
    uint32_t code; /* NEB_CT_NEW, _EXISTING, _DUP, _FULL */
    uint32_t slot; /* where the entry is (every copy of a key reports the same) */
} neb_ct_result;
typedef struct neb_conntrack neb_conntrack;

/* A table of at most `capacity` live entries (1..2^22; fixed: a documented departure, the reference's
 * map has no bound, firewall.go:40). Its slots, 64 bytes each, number the power of two >= 2 x
 * capacity. seed keys the hash, so which flows share a chain is the owner's secret (and a test's
 * choice). tcp_ns, udp_ns, default_ns: the three timeouts (firewall.go:562-569). max_batch (>= 1):
 * the largest n of a batch call; the lookup's device workspace is sized for it here. The rules
 * version starts at 0. e == NULL: a host-only table (the _host calls only), the same image in host
 * memory under the same rules; otherwise the image lives in e's device memory only (the device
 * changes it, so there is no host copy) and only the device calls work. */
NEB_API int neb_conntrack_create(neb_engine* e, uint32_t capacity, uint64_t seed, uint64_t tcp_ns, uint64_t udp_ns,
                                 uint64_t default_ns, uint32_t max_batch, neb_conntrack** out);
/* No call on the table may be in progress; waits for the device work the table has enqueued. */
NEB_API int neb_conntrack_destroy(neb_conntrack* t);
/* f.rulesVersion after a reload: calls enqueued after this returns use v. */
NEB_API int neb_conntrack_set_rules_version(neb_conntrack* t, uint16_t v);
/* inConns per packet i (the localCache argument is a per-routine shortcut with no semantics: no
 * counterpart). status[i] != NEB_STATUS_OK: verdict NEB_CT_NONE, not looked up, nothing else written
 * for it. Otherwise: key absent -> NEB_CT_MISS; present with another rulesVersion -> NEB_CT_STALE
 * [| NEB_CT_INCOMING], the entry untouched: the caller re-matches its rules in that direction and
 * then adds the key again with that incoming, or evicts it with force; else NEB_CT_HIT and Expires =
 * max(Expires, now_ns + timeout(protocol)). now_ns is one reading of a monotonic clock per call,
 * under which the max is the reference's overwrite. An entry past its Expires that nobody has
 * evicted still hits and is refreshed, as in the reference: the table expires nothing by itself.
 * Holding: with d_plain and / or d_tx given, every looked-up packet that is not a HIT gets
 * NEB_PLAIN_SKIP or-ed into d_plain[i].flags, d_tx[i].tunnel = NEB_TX_NO_TUNNEL and d_status[i] =
 * NEB_STATUS_FW_HELD, so the coalescer or the seal that follows on the stream passes the hits on only.
 * With both NULL, d_status is only read.
 * Work list: the MISS and STALE packets in ascending packet order, at most work_cap of them (d_work
 * may be NULL with work_cap == 0). d_counts = {hits, misses, stales, work entries in total, also
 * beyond work_cap}. All packets of one flow in one batch get the same verdict.
 * d_fw, d_work and d_plain are 16-byte aligned. n == 0 returns NEB_OK and enqueues nothing.
 * NEB_ERR_INVALID (nothing launched): n > max_batch, a misaligned or missing array, a host-only
 * table, a table of another engine. */
NEB_API int neb_conntrack_lookup_batch(neb_engine* e, neb_conntrack* t, const neb_fw_packet* d_fw, int32_t* d_status,
                                       uint32_t n, uint64_t now_ns, uint8_t* d_verdict, neb_plain_packet* d_plain,
                                       neb_tx_packet* d_tx, neb_ct_work* d_work, uint32_t work_cap, uint32_t* d_counts,
                                       void* stream);
/* The same over host memory, on a host-only table; any alignment. */
NEB_API int neb_conntrack_lookup_batch_host(neb_conntrack* t, const neb_fw_packet* fw, int32_t* status, uint32_t n,
                                            uint64_t now_ns, uint8_t* verdict, neb_plain_packet* plain, neb_tx_packet* tx,
                                            neb_ct_work* work, uint32_t work_cap, uint32_t* counts);
/* addConn per key i with incoming[i] != 0 as its direction: absent -> {now_ns + timeout, incoming,
 * the current rulesVersion} inserted, NEB_CT_NEW; present -> the three fields overwritten,
 * NEB_CT_EXISTING. Of several copies of one key in a batch exactly one answers NEW or EXISTING, the
 * others NEB_CT_DUP, all with the same slot, and the stored incoming is that of the highest index, as
 * sequential addConn calls would leave it. An add that would take the live count past capacity, or
 * that finds no empty slot (tombstones: compact), answers NEB_CT_FULL, as do all copies of its key;
 * the flow is then untracked and takes the rules path every time. Which of a batch's new keys are
 * refused is unspecified (the host form: the later ones); exactly `capacity` entries are live
 * afterwards. A full table is left as it is; in the batch that fills it, a key that had taken its
 * slot when the last place went leaves that slot a tombstone (the host form: none). Two launches on
 * `stream`, no lane ever waits for another. d_keys is 16-byte aligned, d_result 4-byte. */
NEB_API int neb_conntrack_add_batch(neb_engine* e, neb_conntrack* t, const neb_fw_packet* d_keys, const uint8_t* d_incoming,
                                    uint32_t n, uint64_t now_ns, neb_ct_result* d_result, void* stream);
NEB_API int neb_conntrack_add_batch_host(neb_conntrack* t, const neb_fw_packet* keys, const uint8_t* incoming, uint32_t n,
                                         uint64_t now_ns, neb_ct_result* result);
/* evict per key i (force: the stale entry's delete of firewall.go:545): absent -> -1; Expires >
 * now_ns and force == 0 -> the remaining ns (> 0), the entry stays and the caller re-adds the key to
 * its wheel; otherwise the entry is removed (its slot becomes a tombstone) and the result is 0. Every
 * copy of a duplicated key reports what it found: 0 where the entry was still there, -1 behind the
 * copy that removed it (the host form: the first copy 0, the others -1). d_keys is 16-byte aligned,
 * d_remaining 8-byte. */
NEB_API int neb_conntrack_evict_batch(neb_engine* e, neb_conntrack* t, const neb_fw_packet* d_keys, uint32_t n,
                                      uint64_t now_ns, int force, int64_t* d_remaining, void* stream);
NEB_API int neb_conntrack_evict_batch_host(neb_conntrack* t, const neb_fw_packet* keys, uint32_t n, uint64_t now_ns,
                                           int force, int64_t* remaining);
/* Rehashes every live entry into a cleared image (value fields kept) and switches over: tombstones
 * drop to 0. Blocks until switched; no other call on t meanwhile. Recommended when live +
 * tombstones > 3/4 of the slots. stream is ignored by a host-only table. */
NEB_API int neb_conntrack_compact(neb_conntrack* t, void* stream);
/* out = {live, tombstones, slots}; waits for the table's enqueued work. EmitStats'
 * firewall.conntrack.count is out[0]. */
NEB_API int neb_conntrack_count(neb_conntrack* t, uint64_t out[3]);
/* For tests: the home slot of a key; and the image, nslots x 64 bytes {state, key[5], expires, meta}
 * (conntrack_core.hpp), after the table's enqueued work. nslots must be the table's slot count. */
NEB_API int neb_conntrack_home(const neb_conntrack* t, const neb_fw_packet* key, uint32_t* slot);
NEB_API int neb_conntrack_dump(neb_conntrack* t, void* slots_out, uint32_t nslots);
/* ---- submission queue: many threads' small flushes -> device-sized batches -------------------- */
/* Nebula seals <= 128 packets per TX flush (overlay/batch/tx_batch.go:5, flushSendBatch
 * interface.go:465-487) and opens <= listen.batch = 64 per RX flush (main.go:181, listenOut
 * interface.go:381-413), from `routines` goroutines at once (interface.go:320-335). A queue
 * gathers those flushes into one device batch: each submission's packets are copied into pinned
 * staging, sealed or opened with the other submissions' by one zero-copy kernel launch, and copied
 * back. A batch goes to the device when it holds max_packets, when the next submission would not
 * fit its staging, on neb_queue_flush, or max_delay_us after its first submission. */
typedef struct neb_queue neb_queue;
typedef struct neb_queue_config {
    uint32_t max_packets;  /* packets per device batch (0: 16384) */
    uint32_t max_delay_us; /* a non-empty batch waits at most this long for more (0: 100 us) */
    uint64_t arena_bytes;  /* pinned staging per batch (0: max_packets x 1536) */
    uint32_t depth;        /* staging batches in rotation, 2..16 (0: 3) */
    uint32_t reserved;     /* 0 */
} neb_queue_config;
/* A queue for one algorithm and direction (open = 0: seal, 1: open). cfg may be NULL (defaults). */
NEB_API int neb_queue_create(neb_engine* e, int alg, int open, const neb_queue_config* cfg, neb_queue** out);
/* Sends out what is queued, waits for it, and frees the queue (no submission may be in progress). */
NEB_API int neb_queue_destroy(neb_queue* q);
/* Seal or open n packets of the caller's host arena (any memory) through the queue, blocking until
 * they are done: the arena bytes and statuses are those of neb_seal_batch_host / neb_open_batch_host
 * on the same descriptors. Thread-safe, meant to be called by many threads at once. Every
 * descriptor is checked against arena_len first (NEB_ERR_INVALID: nothing touched). A submission
 * larger than one batch goes through in pieces. An arena from neb_host_alloc (pinned, mapped) is
 * not copied: only its descriptors are staged and the kernels work on its bytes in place
 * (zero-copy), so it must stay allocated until the call returns; any other memory is copied
 * into the queue's staging and back. */
NEB_API int neb_queue_submit(neb_queue* q, const neb_desc* desc, uint32_t n, uint8_t* arena, size_t arena_len,
                             int32_t* status);
/* Send the batch being filled to the device now, without waiting for its deadline. */
NEB_API int neb_queue_flush(neb_queue* q);
/* stats[0..3]: device batches launched, packets, submissions, staged bytes (since creation). */
NEB_API int neb_queue_stats(neb_queue* q, uint64_t stats[4]);
/* Where a submission's time goes, in nanoseconds summed since creation: per device batch ns[0] fill
 * (first submission -> sealed), ns[1] drain (sealed -> launched: the last copy-ins), ns[2] device
 * (launched -> done: launch, kernel, completion); per submission ns[3] copy-in, ns[4] wait (copy-in
 * done -> its batch done), ns[5] copy-out. Divide by neb_queue_stats' batches / submissions. */
NEB_API int neb_queue_phases(neb_queue* q, uint64_t ns[6]);

/* ---- header (the AAD) --------------------------------------------------------------------- */

NEB_API void neb_header_encode(uint8_t b[16], uint8_t version, uint8_t type, uint8_t subtype, uint32_t remote_index,
                               uint64_t counter);
/* Returns NEB_ERR_INVALID when len < 16 (ErrHeaderTooShort). */
NEB_API int neb_header_parse(const uint8_t* b, size_t len, uint8_t* version, uint8_t* type, uint8_t* subtype,
                             uint16_t* reserved, uint32_t* remote_index, uint64_t* counter);

#ifdef __cplusplus
}
#endif
#endif /* NEBULA_AEAD_H */
