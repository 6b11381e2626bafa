/* fdgpu_engine.h -- what the host engine's units share (fdgpu_engine.cpp, fdgpu_ring.cpp, fdgpu_frags.cpp,
   fdgpu_expand.cpp, fdgpu_dev_batch.cpp, fdgpu_sync.cpp, fdgpu_diag.cpp, fdgpu_shreds.cpp, fdgpu_shred_sets.cpp, fdgpu_poh_batch.cpp, fdgpu_precompiles.cpp, fdgpu_secp256k1s.cpp): the error text, the environment switches,
   the owners of HIP memory, the ring's slot and the engine, the host-side buffer layouts, and the few internals more
   than one unit calls.  Everything here has hidden visibility: the exported C ABI is include/fd_ed25519_gpu.h and its
   extensions include/fd_shred_gpu.h, include/fd_shred_sets_gpu.h, include/fd_poh_gpu.h, include/fd_precompile_gpu.h and include/fd_secp256k1_gpu.h, nothing else (tests/test_abi.py).  The kernels do not include this file. */
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fd_ed25519_gpu.h"
#include "../../include/fd_poh_gpu.h"
#include "../../include/fd_precompile_gpu.h"
#include "../../include/fd_secp256k1_gpu.h"
#include "../../include/fd_shred_gpu.h"
#include "../../include/fd_shred_sets_gpu.h"
#include "fdgpu_internal.h"
#include "fdt_parse.h"

#define FDT_TXN_MAX_SZ_BYTES 852u   /* FD_TXN_MAX_SZ (fd_txn.h:98): one parsed fd_txn_t record */
#define FDT_TXN_MTU_BYTES 1232u     /* FD_TXN_MTU (fd_txn.h:103) */

#pragma GCC visibility push(hidden)

namespace fdgpu {

inline thread_local std::string g_err;   /* fdgpu_last_error() of this thread */

inline void set_err(const char *fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  g_err = buf;
}

#define HIPCHK(x, ret) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
  set_err("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); return ret; } } while (0)

inline uint64_t sp_now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1000000000ull + ts.tv_nsec; }

/* The one parser of environment values; `v` is getenv's answer.  env_is: the value starts with c ('1' or '0');
   env_eq: it is s.  env_num: a number (strtoll: decimal, or any base with base 0), dflt when unset; the caller
   applies the bounds. */
inline bool env_is(const char *v, char c) { return v && v[0] == c; }
inline bool env_eq(const char *v, const char *s) { return v && !strcmp(v, s); }
inline long long env_num(const char *v, long long dflt, int base = 10) { return v ? strtoll(v, nullptr, base) : dflt; }

/* Every switch the engine reads from the environment, with its default (the synchronous API's four are SyncEnv in
   fdgpu_sync.cpp; the kernels' own FDGPU_AUX_BLOCKS_IN / _FIN stay in fdgpu_ingest.hip).  Constructing an Env reads
   them all; the moment a switch counts is the moment of the Env it is taken from:
     load  g_env, constructed when the library is loaded
     open  a fresh Env in each fdgpu_engine_open (and, for the two debug ones, in each fdgpu_build_info) */
struct Env {
  /* load: off; fdgpu_submit_frags_io's time (validation loop, enqueue) is printed at engine close */
  bool submit_prof = env_is(getenv("FDGPU_SUBMIT_PROF"), '1');
  /* load: off; gathered batches read their payloads by DMA into a device mirror (fdgpu_frags.cpp) */
  bool io_dma = env_is(getenv("FDGPU_IO_DMA"), '1');
  /* load: on; 0: big ring batches verify on their own slot streams (A/B) */
  bool big_streams = !env_is(getenv("FDGPU_BIG_STREAMS"), '0');
  /* load: per engine; "device": the auto flags weigh every engine open on the device */
  bool auto_device_scope = env_eq(getenv("FDGPU_AUTO_SCOPE"), "device");
  /* load: 16 MB; the staging upload piece (A/B); 0 or less: one piece per copy thread */
  uint64_t copy_chunk = [] { const long long m = env_num(getenv("FDGPU_COPY_CHUNK_MB"), 16);
                             return m > 0 ? (uint64_t)m << 20 : UINT64_MAX; }();
  /* open: off; polls ask hipEventQuery, no completion words */
  bool poll_event = env_is(getenv("FDGPU_POLL_EVENT"), '1');
  /* open: two merge streams; 1: one */
  uint32_t merge_streams = env_is(getenv("FDGPU_MERGE_STREAMS"), '1') ? 1u : 2u;
  /* open: off; test hook: completion words are never written, polls finish through the event */
  bool drop_flag = env_is(getenv("FDGPU_DEBUG_DROP_FLAG"), '1');
  /* open: 0; test hook: the k-th merge launch fails before it queues anything */
  int fail_merge = (int)env_num(getenv("FDGPU_DEBUG_FAIL_MERGE"), 0);
};
extern const Env g_env;   /* fdgpu_engine.cpp */

/* Owners of hipMalloc (DevBuf) and hipHostMalloc (HostBuf) memory: freed with the owner, movable (so a Slot is),
   converting to the pointer held. */
template <class T, bool Host> struct HipBuf {
  T *p = nullptr;
  HipBuf() = default;
  HipBuf(HipBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
  HipBuf &operator=(HipBuf &&o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
  ~HipBuf() { reset(); }
  void reset() { if (p) (void)(Host ? hipHostFree(p) : hipFree(p)); p = nullptr; }
  hipError_t alloc(size_t bytes) {
    reset();
    const hipError_t rc = Host ? hipHostMalloc((void **)&p, bytes, hipHostMallocDefault) : hipMalloc((void **)&p, bytes);
    if (rc != hipSuccess) p = nullptr;
    return rc;
  }
  operator T *() const { return p; }
};
template <class T> using DevBuf = HipBuf<T, false>;
template <class T> using HostBuf = HipBuf<T, true>;

/* A batch's arena resident on the device for the synchronous paths (the diagnostics, fdgpu_dev_batch_upload*): arena_sz
   + extra + FDGPU_ARENA_SLACK bytes, zeroed -- all of them, or only those past the arena -- with the arena copied in. */
inline hipError_t dev_arena(DevBuf<uint8_t> &d, uint8_t const *arena, uint64_t arena_sz, uint64_t extra = 0,
                            bool zero_all = true) {
  const uint64_t bytes = arena_sz + extra + FDGPU_ARENA_SLACK, z0 = zero_all ? 0 : arena_sz;
  hipError_t rc = d.alloc(bytes);
  if (rc == hipSuccess) rc = hipMemset(d.p + z0, 0, bytes - z0);
  if (rc == hipSuccess && arena_sz) rc = hipMemcpy(d, arena, arena_sz, hipMemcpyHostToDevice);
  return rc;
}

/* N timing events: create makes all of them or none (what it made before a failure is destroyed), and they go with
   their owner. */
struct Events {
  std::vector<hipEvent_t> ev;
  Events() = default;
  Events(const Events &) = delete;
  Events &operator=(const Events &) = delete;
  ~Events() { clear(); }
  void clear() { for (hipEvent_t x : ev) (void)hipEventDestroy(x); ev.clear(); }
  bool create(size_t n) {
    clear();
    while (ev.size() < n) {
      hipEvent_t x;
      if (hipEventCreate(&x) != hipSuccess) { clear(); return false; }
      ev.push_back(x);
    }
    return true;
  }
  hipEvent_t operator[](size_t i) const { return ev[i]; }
};

/* The device-side parse buffers of a frag batch of up to n_txn payloads (fdgpu_launch_frag_ingest and its kin): n_txn
   + 1 entries each, and the scan's block totals.  alloc returns null, or what could not be allocated. */
struct ParseBufs {
  DevBuf<uint8_t> txn_out;       /* FDT_TXN_MAX_SZ_BYTES per txn: the parsed fd_txn_t records */
  DevBuf<uint16_t> txn_sz;
  DevBuf<fdgpu_txn_t> txd;
  DevBuf<uint32_t> cnt, sig0, blocktot, n_sig;
  const char *alloc(uint64_t n_txn) {
    const uint64_t n = n_txn + 1, nb = (n_txn + 1023) / 1024 + 2;
    if (txn_out.alloc(n * FDT_TXN_MAX_SZ_BYTES) || txn_sz.alloc(n * sizeof(uint16_t)) || txd.alloc(n * sizeof(fdgpu_txn_t)))
      return "txn alloc";
    if (cnt.alloc(n * sizeof(uint32_t)) || sig0.alloc(n * sizeof(uint32_t)) || blocktot.alloc(nb * sizeof(uint32_t)) ||
        n_sig.alloc(sizeof(uint32_t)))
      return "scan alloc";
    return nullptr;
  }
};

/* A gathered batch's results for n frags, in the slot's pinned h_tr (the finish kernel writes them in place): [codes,
   padded to 64][8 B tags][2 B out sizes]. */
struct IoResults { uint64_t tags, sizes, bytes; };
inline IoResults io_results(uint64_t n) {
  const uint64_t cb = (n + 63) & ~63ull;
  return {cb, cb + n * 8, cb + n * 10};
}

/* An item batch's results for n items (a shred's root, a PoH entry's hash: 32 B; a precompile transaction's info:
   16 B), in the slot's d_res and its pinned read-back h_res: [codes, padded to 64][item_sz B per item]. */
struct ItemResults { uint64_t items, bytes; };
inline ItemResults item_results(uint64_t n, uint64_t item_sz = 32) {
  const uint64_t cb = (n + 63) & ~63ull;
  return {cb, cb + n * item_sz};
}

/* A set batch's results for n shreds (fdgpu_submit_shred_sets), in the slot's d_sres and its pinned read-back h_sres:
   [codes, padded to 64][32 B roots][4 B representatives][the lane count, 4 B, and 12 B of padding]. */
struct SetResults { uint64_t roots, rep, lanes, bytes; };
inline SetResults set_results(uint64_t n) {
  const uint64_t cb = (n + 63) & ~63ull;
  return {cb, cb + 32 * n, cb + 36 * n, cb + 36 * n + 16};
}

/* A gathered batch's pinned record area for n frags (h_io, read in place by the ingest kernel), each part 64-B
   aligned: the frag records at 0, the payloads' device-side addresses, the re-check pairs {mcache line address, seq},
   the DMA gather's range table.  bytes keeps the 192 B of slack the earlier size formula had, so no allocation
   shrinks. */
struct IoRecords { uint64_t src, chk, rtab, bytes; };
inline IoRecords io_records(uint64_t n) {
  auto up64 = [](uint64_t b) { return (b + 63) & ~63ull; };
  const uint64_t src = up64(n * sizeof(fdgpu_frag_ex_t)), chk = src + up64(n * sizeof(uint64_t)),
                 rtab = chk + up64(n * 2 * sizeof(uint64_t));
  return {src, chk, rtab, rtab + FDGPU_IO_RANGES_MAX * sizeof(uint64_t) + 192};
}

enum class Batch : uint8_t {
  Ring,     /* fdgpu_submit / fdgpu_stage_submit: codes in h_codes */
  Frag,     /* fdgpu_submit_frags: [codes][trailers] in h_tr */
  FragIo,   /* fdgpu_submit_frags_io: io_results() in h_tr */
  Shred,    /* fdgpu_submit_shreds: item_results() in h_res, the items the roots */
  Poh,      /* fdgpu_submit_poh: item_results() in h_res, the items the hashes */
  Precompile,   /* fdgpu_submit_precompiles: item_results(n, 16) in h_res, the items the infos */
  Secp256k1,    /* fdgpu_submit_secp256k1: the same */
  ShredSets,    /* fdgpu_submit_shred_sets: set_results() in h_sres */
};

struct Slot {
  hipStream_t stream = nullptr;
  hipEvent_t h2d_done = nullptr, comp_done = nullptr, done = nullptr;
  HostBuf<uint8_t> h_arena; DevBuf<uint8_t> d_arena;
  HostBuf<fdgpu_sig_desc_t> h_sigs; DevBuf<fdgpu_sig_desc_t> d_sigs;
  HostBuf<uint32_t> h_perm;       /* block-count grouping: descriptor i -> signature perm[i] */
  DevBuf<uint32_t> d_perm;
  HostBuf<fdgpu_txn_desc_t> h_txns; DevBuf<fdgpu_txn_desc_t> d_txns;
  HostBuf<int8_t> h_codes;
  DevBuf<int8_t> d_txn_codes, d_sig_codes;
  DevBuf<uint32_t> d_ws;      /* this slot's workspace: slots run concurrently on their own streams; */
  uint64_t ws_sig = 0;        /* sized on demand to the largest batch the slot has carried */
  int64_t ticket = -1;      /* -1: free */
  uint64_t k_sigs = 0;      /* signatures (the launch's bound) of its verify: FDGPU_FLAG_PAIR_AUTO's load */
  uint64_t k_lanes = 0;     /* and its lanes (two per signature for the two-lane kernel): FDGPU_FLAG_SPREAD_AUTO's */
  bool staged = false;      /* reserved by fdgpu_stage_acquire, not yet submitted */
  bool held = false;        /* polled with fdgpu_poll_keep, awaiting fdgpu_release */
  uint64_t txn_cnt = 0;
  /* completion word in pinned host memory: the slot's stream writes flag_seq into it after the code read-back
     (hipStreamWriteValue32), so a non-blocking poll is one host load instead of a runtime event query */
  HostBuf<uint32_t> h_flag;
  uint32_t *d_flag = nullptr;
  uint32_t flag_seq = 0;
  uint32_t polls = 0;         /* non-blocking polls of the current batch (stream error checks) */
  uint64_t last_query = 0;    /* when a poll last asked the runtime (ns) */
  Batch kind = Batch::Ring;   /* of the batch in flight: what poll_slot reads back */
  /* frag batches (fdgpu_submit_frags): GPU-side parse buffers, allocated on the slot's first frag batch; the trailer
     buffers grow to the batches */
  HostBuf<fdgpu_frag_ex_t> h_fx; DevBuf<fdgpu_frag_ex_t> d_fx;
  ParseBufs pb;
  DevBuf<uint8_t> d_tr;       /* [codes, padded to 64][trailers]: one read-back */
  HostBuf<uint8_t> h_tr;
  uint64_t tr_cap = 0, tr_sz = 0, tr_base = 0;
  /* gathered frag batches (fdgpu_submit_frags_io): the payloads' device-side addresses, and the out image the finish
     kernel assembles (grown on demand); the read-back is io_results() in h_tr */
  HostBuf<uint8_t> h_io;                      /* pinned io_records() */
  uint8_t *d_ioh = nullptr;                   /* its device view */
  DevBuf<fdgpu_frag_ex_t> d_fxio;             /* the records, kept on the device by the ingest */
  DevBuf<uint32_t> d_io_cnt;                  /* the ingest's signature count: zero at the start of a gathered
                                                 batch (cleared by the finish of the slot's previous one) */
  bool io_cnt_dirty = false;                  /* an ingest was queued but not its finish (an error between
                                                 them): the next gathered batch clears the count first */
  DevBuf<uint8_t> d_mirror;                   /* DMA gather: the batch's source ranges, copied in by the DMA
                                                 engines, parsed and verified in place (the batch arena) */
  uint64_t mirror_cap = 0;
  uint8_t *d_trh = nullptr;                   /* h_tr's device-side address (results written in place) */
  /* shred, PoH and precompile batches: item_results() of max_txn + 1 items (32 B each, which holds a precompile
     batch's 16) and their pinned read-back, allocated on the slot's first batch of any of them (slot_res_bufs) */
  DevBuf<uint8_t> d_res; HostBuf<uint8_t> h_res;
  /* shred batches (fdgpu_submit_shreds), allocated on the slot's first one for max_txn shreds: the records and the
     ingest's signature count */
  HostBuf<fdgpu_shred_t> h_sh; DevBuf<fdgpu_shred_t> d_sh;
  DevBuf<uint32_t> d_sh_cnt;
  /* set batches (fdgpu_submit_shred_sets), allocated on the slot's first one for max_txn shreds: the records, the
     states, the dedup's table (a power of two >= 2 (max_txn + 1) words), the representatives' descriptor slots, the
     dedup's signature count, and set_results() with its pinned read-back */
  HostBuf<fdgpu_set_shred_t> h_set; DevBuf<fdgpu_set_shred_t> d_set;
  DevBuf<uint8_t> d_set_state;
  DevBuf<uint32_t> d_set_ht, d_set_slot, d_set_cnt;
  DevBuf<uint8_t> d_sres; HostBuf<uint8_t> h_sres;
  /* PoH batches (fdgpu_submit_poh), allocated on the slot's first one for max_txn entries and max_sig signatures:
     the entries, the signatures' arena offsets, the queue (entry indices, longest chain first) and its head, and the
     tree's nodes (32 B per signature) */
  HostBuf<fdgpu_poh_entry_t> h_pe; DevBuf<fdgpu_poh_entry_t> d_pe;
  HostBuf<uint32_t> h_psig, h_pord; DevBuf<uint32_t> d_psig, d_pord, d_pnodes, d_phead;
  /* precompile batches (fdgpu_submit_precompiles, fdgpu_submit_secp256k1), allocated on the slot's first one for max_txn transactions and
     max_sig signatures: the records, the ingest's signature count, the parsed fd_txn_t records (FDT_TXN_MAX_SZ_BYTES
     each), the walks' outcomes and the signatures' positions */
  HostBuf<fdgpu_precompile_t> h_pc; DevBuf<fdgpu_precompile_t> d_pc;
  DevBuf<uint32_t> d_pc_cnt, d_pc_pos;
  DevBuf<uint8_t> d_pc_txn;
  DevBuf<fdgpu_precompile_walk_t> d_pc_walk;
  /* FDGPU_FLAG_MERGE: the batch's gather + parse are queued and its verify waits to be merged with the other batches
     ready (merge_kick), which then queues the rest of the batch behind it */
  hipEvent_t parsed = nullptr;
  bool vpending = false;
  bool failed = false;        /* its merged verify could not be queued: the next poll reports the error */
  uint32_t m_n = 0;
  uint64_t m_seed = 0, m_bound = 0;
  uint8_t *m_out = nullptr;
  uint8_t *m_arena = nullptr;   /* the batch arena (d_arena, or d_mirror for a DMA-gathered batch) */
};

/* poll_slot answers a pending batch without the ring lock, reading a slot's ticket, held, flag_seq and polls
   atomically; every write of those fields (under ring_mu) is an atomic store too, so the two sides never race */
template <class T> inline void st_rlx(T &f, T v) { __atomic_store_n(&f, v, __ATOMIC_RELAXED); }

/* a merge stream of an FDGPU_FLAG_MERGE engine */
struct Merge {
  hipStream_t stream = nullptr;
  HostBuf<uint32_t> h_flag; uint32_t *d_flag = nullptr;   /* seq after each merged verify: free when equal */
  uint32_t seq = 0;
  HostBuf<fdgpu_mbatch_t> h_tab; fdgpu_mbatch_t *d_tab = nullptr;   /* tabs x ring_depth batch entries, pinned */
  std::vector<hipEvent_t> ev;                          /* one per table: the launch that read it is done */
};

}  // namespace fdgpu

struct fdgpu_engine {
  int device = 0;
  fdgpu_cfg_t cfg{};
  hipStream_t compute = nullptr;
  uint32_t *d_btab = nullptr;
  fdgpu::DevBuf<uint32_t> d_ws;      /* per-lane A-table workspace, fdgpu_ws_bytes(ws_sig) */
  size_t ws_bytes = 0;
  uint64_t ws_sig = 0;
  uint32_t resident_blocks = 0;     /* verify-kernel occupancy x CUs (fallback grid cap, reporting) */
  uint64_t kc_seed = 0;             /* key cache hash seed, drawn at open */
  std::vector<fdgpu::Slot> slots;
  int64_t next_ticket = 0;
  fdgpu::DevBuf<int8_t> d_scratch_codes;   /* for fdgpu_verify_device with d_sig_codes == NULL */
  uint64_t scratch_cap = 0;
  std::vector<hipStream_t> batch_streams;   /* streams of device batches with their own queue */
  /* ring batches that fill the chip on their own (FDGPU_BIG_SIGS) verify on these two streams in turn, not on their
     slot's: see submit_slot */
  hipStream_t big[2] = {nullptr, nullptr};
  uint32_t big_rr = 0;
  /* the ring API (submit / stage / poll / release) may be called from several host threads (verify tiles sharing the
     node's engines) */
  std::mutex ring_mu;
  bool flag_poll = false;            /* slots signal completion through h_flag (probed at open) */
  /* fdgpu_host_register calls of this engine, one entry each (a range registered twice holds two references): the
     page-aligned start the caller named, and the pinned region [base, end) that covers it */
  struct Reg { uintptr_t user, base, end, dbase; };   /* dbase: the region's device-side address */
  std::vector<Reg> regions;
  bool drop_flag = false;            /* Env::drop_flag at open: polls must finish through the event */
  uint32_t fail_merge_at = 0;        /* Env::fail_merge at open: that merge launch fails before queueing
                                        anything, as a HIP error part-way would */
  uint32_t merge_calls = 0;
  /* FDGPU_FLAG_MERGE */
  std::vector<fdgpu::Merge> merges;
  std::vector<fdgpu::Slot *> pending;   /* batches parsed (or parsing) whose verify is not launched */
  uint32_t merge_rr = 0, merge_tabs = 0;
  uint64_t merge_launches = 0, merge_batches = 0;
};

namespace fdgpu {

#ifndef FDGPU_COPY_THREADS_N
#define FDGPU_COPY_THREADS_N 4                 /* A/B builds may change it */
#endif
constexpr unsigned FDGPU_COPY_THREADS = FDGPU_COPY_THREADS_N;

inline bool bucket(const fdgpu_engine_t *e) { return !(e->cfg.flags & FDGPU_FLAG_NO_BUCKET); }

/* fdgpu_engine.cpp */
uint32_t kflags(const fdgpu_engine_t *e);                          /* the kernels' flags for the engine's configuration */
uint32_t ring_kflags(fdgpu_engine_t *e, Slot *s, uint64_t n_sig);  /* ... of slot s's ring batch (ring_mu held) */
bool slot_ws(Slot &s, uint64_t n_sig);
bool slot_frag_bufs(Slot &s, const fdgpu_cfg_t &c, uint64_t tr);
bool slot_io_bufs(Slot &s, const fdgpu_cfg_t &c);
bool slot_res_bufs(Slot &s, const fdgpu_cfg_t &c);
const fdgpu_engine::Reg *region_of(const fdgpu_engine *e, uintptr_t p, uint64_t sz);
int ensure_ws(fdgpu_engine *e, uint64_t n_sig);
int enqueue_verify(fdgpu_engine_t *e, const uint8_t *d_arena, const fdgpu_sig_desc_t *d_sigs, const uint32_t *d_perm,
                   uint64_t n_sig, const fdgpu_txn_desc_t *d_txns, uint64_t n_txn, int8_t *d_sig_codes,
                   int8_t *d_txn_codes, hipStream_t st, uint32_t *ws = nullptr, uint32_t flags = ~0u);

/* fdgpu_ring.cpp */
int take_slot(fdgpu_engine_t *e, Slot **s);
int slot_upload(fdgpu_engine_t *e, Slot *s, uint8_t const *arena, uint64_t arena_sz);
int slot_signal(fdgpu_engine_t *e, Slot *s);
int64_t slot_publish(fdgpu_engine_t *e, Slot *s, Batch kind, uint64_t txn_cnt, uint64_t tr_sz, uint64_t tr_base,
                     bool signal_deferred = false);
/* the poll of every batch kind: what the kind does not produce stays unwritten (items: a shred or set batch's roots, a
   PoH batch's hashes, a precompile batch's infos; rep, lanes: a set batch's representatives and lane count) */
int poll_slot(fdgpu_engine_t *e, int64_t ticket, int8_t *txn_codes, int blocking, bool keep, uint8_t *trailers = nullptr,
              uint64_t *tags = nullptr, uint16_t *out_szs = nullptr, uint8_t *items = nullptr, uint32_t *rep = nullptr,
              uint64_t *lanes = nullptr);

/* fdgpu_precompiles.cpp: what both precompile batch kinds (fdgpu_precompiles.cpp, fdgpu_secp256k1s.cpp) share */
int precompile_args(const fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_precompile_t const *tx,
                    uint64_t n, uint64_t *sig_cap);
bool slot_precompile_bufs(Slot &s, const fdgpu_cfg_t &c);

/* fdgpu_frags.cpp */
int merge_kick(fdgpu_engine_t *e, bool force);
void submit_prof_report();                     /* Env::submit_prof: the totals so far, to stderr */

/* fdgpu_diag.cpp */
int time_two_stages(hipStream_t st, int iters, const char *what, const std::function<bool()> &warm,
                    const std::function<bool()> &first, const std::function<bool()> &second, double *first_ms,
                    double *second_ms);

/* fdgpu_expand.cpp */
int64_t expand(uint64_t arena_sz, const fdgpu_txn_t *txns, uint64_t txn_cnt, uint64_t max_sig, fdgpu_sig_desc_t *sigs,
               fdgpu_txn_desc_t *tds, uint32_t *perm);
int64_t expand_par(uint64_t arena_sz, const fdgpu_txn_t *txns, uint64_t txn_cnt, uint64_t max_sig,
                   fdgpu_sig_desc_t *sigs, fdgpu_txn_desc_t *tds, uint32_t *perm);
/* runs fns[1..] on the process-wide copy threads and fns[0] here, one caller at a time; returns when all are done */
void copy_run(std::vector<std::function<void()>> &fns);

}  // namespace fdgpu

#pragma GCC visibility pop
