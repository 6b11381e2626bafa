/* fdgpu_engine.cpp -- the core of the host side of the MI355X Ed25519 verify engine (the exported C ABI is
   include/fd_ed25519_gpu.h): an engine's lifetime and buffers; fdgpu_engine.h names the other units.

   Per engine (one per GPU):
     - `ring_depth` staging slots, each with pinned host buffers, device
       buffers, its own stream and its own workspace: a slot's H2D copy,
       verify kernels and D2H of the codes run in order on its stream, and
       the slots' batches overlap each other on the GPU (copies of one batch
       under the kernels of another; two small batches sharing the CUs);
     - one compute stream + workspace for the device-resident path
       (fdgpu_dev_batch_*, fdgpu_verify_device) and the diagnostics;
     - the fixed-base comb table (built on the device at open). */
#include <algorithm>
#include <map>
#include <random>

#include "fdgpu_engine.h"

using namespace fdgpu;

namespace fdgpu {
const Env g_env;                               /* read when the library is loaded */
}

namespace {

void slot_free(Slot &s) {
  if (s.stream) (void)hipStreamDestroy(s.stream);
  for (hipEvent_t ev : {s.h2d_done, s.comp_done, s.done, s.parsed})
    if (ev) (void)hipEventDestroy(ev);
  s = Slot{};                                  /* its buffers go with their owners */
}

bool slot_alloc(Slot &s, const fdgpu_cfg_t &c) {
  const size_t arena = c.max_arena + FDGPU_ARENA_SLACK;
  HIPCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking), false);
  HIPCHK(hipEventCreateWithFlags(&s.h2d_done, hipEventDisableTiming), false);
  HIPCHK(hipEventCreateWithFlags(&s.comp_done, hipEventDisableTiming), false);
  HIPCHK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming), false);
  HIPCHK(hipEventCreateWithFlags(&s.parsed, hipEventDisableTiming), false);
  HIPCHK(s.h_arena.alloc(arena), false);
  HIPCHK(s.h_sigs.alloc(c.max_sig * sizeof(fdgpu_sig_desc_t) + 16), false);
  HIPCHK(s.h_perm.alloc(c.max_sig * sizeof(uint32_t) + 16), false);
  HIPCHK(s.h_txns.alloc(c.max_txn * sizeof(fdgpu_txn_desc_t) + 16), false);
  HIPCHK(s.h_codes.alloc(c.max_txn + 16), false);
  HIPCHK(s.d_arena.alloc(arena), false);
  HIPCHK(s.d_sigs.alloc(c.max_sig * sizeof(fdgpu_sig_desc_t) + 16), false);
  HIPCHK(s.d_perm.alloc(c.max_sig * sizeof(uint32_t) + 16), false);
  HIPCHK(s.d_txns.alloc(c.max_txn * sizeof(fdgpu_txn_desc_t) + 16), false);
  HIPCHK(s.d_txn_codes.alloc(c.max_txn + 16), false);
  HIPCHK(s.d_sig_codes.alloc(c.max_sig + 16), false);
  HIPCHK(s.h_flag.alloc(64), false);           /* own cache line */
  *s.h_flag = 0;
  HIPCHK(hipHostGetDevicePointer((void **)&s.d_flag, s.h_flag, 0), false);
  return true;
}

/* DMA gather: the batch's ranges may also carry other tiles' frags lying between this batch's (a round robin of two
   takes every other frag of a link), so the mirror holds twice the engine's arena */
inline uint64_t mirror_bytes(const fdgpu_cfg_t &c) { return 2 * c.max_arena + FDGPU_ARENA_SLACK + 4096; }

/* The fixed-base comb table is a device constant (67 MB): one copy per device, shared by every engine opened on it
   (refcounted), so engines of several verify tiles on one GPU read the same lines from the Infinity Cache instead of
   each streaming its own copy. */
std::mutex g_btab_mu;
std::map<int, std::pair<uint32_t *, int>> g_btab;

uint32_t *btab_acquire(int device, hipStream_t st) {
  std::lock_guard<std::mutex> lk(g_btab_mu);
  auto it = g_btab.find(device);
  if (it != g_btab.end()) { it->second.second++; return it->second.first; }
  uint32_t *p = nullptr;
  if (hipMalloc((void **)&p, fdgpu_btab_bytes()) != hipSuccess) { set_err("btab alloc"); return nullptr; }
  if (fdgpu_btab_build(p, st) != hipSuccess) { (void)hipFree(p); set_err("fixed-base table build failed"); return nullptr; }
  g_btab[device] = {p, 1};
  return p;
}

void btab_release(int device, uint32_t *p) {
  std::lock_guard<std::mutex> lk(g_btab_mu);
  auto it = g_btab.find(device);
  if (it == g_btab.end() || it->second.first != p) return;
  if (--it->second.second == 0) { (void)hipFree(p); g_btab.erase(it); }
}

/* Host regions registered for direct DMA (hipHostRegister, portable to every device), reference-counted across the
   engines that registered them: page-aligned base -> end, references over every engine's registrations, and the
   device-side address of base (regions are mapped, so kernels read them in place: fdgpu_submit_frags_io) */
std::mutex g_reg_mu;
struct GReg { uintptr_t end; int refs; uintptr_t dbase; };
std::map<uintptr_t, GReg> g_regions;

/* drop one reference to the pinned region at base */
void region_release(int device, uintptr_t base) {
  std::lock_guard<std::mutex> rk(g_reg_mu);
  auto it = g_regions.find(base);
  if (it == g_regions.end()) return;
  if (--it->second.refs == 0) {
    (void)hipSetDevice(device);
    (void)hipHostUnregister((void *)base);
    g_regions.erase(it);
  }
}

/* FDGPU_FLAG_PAIR_AUTO: a ring batch takes the two-lane kernel while the signatures of the engine's running batches
   and its own (launch bounds: a gathered batch's count is known only on the device), two lanes each, leave part of
   the chip's resident lanes idle (256 CUs x 4 SIMDs x 2 waves x 64 = 131,072): a wave's lifetime is then the batch's
   latency (profiles/r04/pair_rocprof.txt: 0.73x the one-lane kernel's time at 4-16 K signatures, 0.76x at 32 K;
   pair_probe.jsonl: 1.2x at 64 K, where two lanes per signature fill the chip).  A loaded engine keeps the one-lane
   kernel, which does ~1.4x less work per signature. */
constexpr uint64_t FDGPU_PAIR_AUTO_SIGS = 49152;

/* FDGPU_FLAG_SPREAD_AUTO: a ring batch's verify blocks take one CU each (FDGPU_FLAG_KSPREAD: dynamic LDS that leaves
   no room for a second block) while its lanes and those of the engine's running batches fit the chip one block per CU
   (256 CUs x 256 lanes).  Concurrent launches from other streams otherwise stack two blocks on a CU while other CUs
   idle: four 16 K launches at once verify 82 M sigs/s spread against 55 M packed, but spread caps the chip at ~89 M
   where packing reaches 106 M with 12+ launches (profiles/r04/spread.md). */
constexpr uint64_t FDGPU_SPREAD_AUTO_LANES = 65536;

/* The auto flags can weigh the running batches of every engine open on the device, not only the caller's: each verify
   tile has an engine of its own, and two tiles at capacity each saw about half the chip's load -- each kept spreading
   its verifies one block per CU (and taking the two-lane kernel) while the chip was full.  Measured, that view is the
   worse one: two tiles at capacity 58.8 vs 60.1 M txn/s and, paced at 24 M, p50 / p99 batch latency 1.31 / 1.78 vs
   0.97 / 1.07 ms (profiles/r05/auto_scope.md), so the per-engine view stays the default and Env::auto_device_scope
   selects this one.  Other engines' slots are read without their locks: the fields are atomics, and a stale view only
   shifts the estimate by a batch. */
std::mutex g_dev_mu;
std::map<int, std::vector<fdgpu_engine_t *>> g_dev_eng;

/* signatures and lanes of o's running batches (s excluded) into load, lanes */
void running_load(const fdgpu_engine_t *o, const Slot *s, uint64_t &load, uint64_t &lanes) {
  for (const auto &c : o->slots) {
    if (&c == s || __atomic_load_n(&c.ticket, __ATOMIC_RELAXED) < 0) continue;
    if (o->flag_poll && __atomic_load_n(c.h_flag.p, __ATOMIC_ACQUIRE) == __atomic_load_n(&c.flag_seq, __ATOMIC_RELAXED))
      continue;                                                      /* complete, not yet polled */
    load += __atomic_load_n(&c.k_sigs, __ATOMIC_RELAXED);
    lanes += __atomic_load_n(&c.k_lanes, __ATOMIC_RELAXED);
  }
}

}  // namespace

namespace fdgpu {

/* Grow the slot's workspace to cover n_sig signatures (the slot is free, so nothing of its stream still reads the old
   one).  Grown by half again each time, so a default engine (65,536 txns, up to 12 signatures each) holds what its
   batches actually carry, not 12 x 3.2 KB per txn up front. */
bool slot_ws(Slot &s, uint64_t n_sig) {
  if (s.d_ws && n_sig <= s.ws_sig) return true;
  const uint64_t want = std::max<uint64_t>(n_sig, s.ws_sig + s.ws_sig / 2);
  if (s.d_ws) { HIPCHK(hipStreamSynchronize(s.stream), false); s.d_ws.reset(); s.ws_sig = 0; }
  if (s.d_ws.alloc(fdgpu_ws_bytes(want ? want : 1)) != hipSuccess) {
    if (want == n_sig || s.d_ws.alloc(fdgpu_ws_bytes(n_sig ? n_sig : 1)) != hipSuccess) {
      (void)hipGetLastError();
      set_err("slot workspace alloc (%llu signatures)", (unsigned long long)n_sig);
      return false;
    }
    s.ws_sig = n_sig ? n_sig : 1;
    return true;
  }
  s.ws_sig = want ? want : 1;
  return true;
}

/* The slot's GPU-side parse buffers (first frag batch) and a trailer buffer of at least tr bytes (the slot is free:
   nothing reads them). */
bool slot_frag_bufs(Slot &s, const fdgpu_cfg_t &c, uint64_t tr) {
  if (!s.d_fx) {
    const uint64_t n = c.max_txn + 1;
    HIPCHK(s.h_fx.alloc(n * sizeof(fdgpu_frag_ex_t)), false);
    HIPCHK(s.d_fx.alloc(n * sizeof(fdgpu_frag_ex_t)), false);
    if (const char *what = s.pb.alloc(c.max_txn)) { set_err("slot parse buffers: %s", what); return false; }
  }
  tr += (c.max_txn + 64) & ~63ull;                      /* the codes go in front of the trailers */
  if (tr > s.tr_cap) {
    HIPCHK(hipStreamSynchronize(s.stream), false);
    s.d_tr.reset();
    s.h_tr.reset();
    s.tr_cap = 0;
    const uint64_t want = std::max<uint64_t>(tr + tr / 4, 256 * 1024);
    HIPCHK(s.d_tr.alloc(want), false);
    HIPCHK(s.h_tr.alloc(want), false);
    HIPCHK(hipHostGetDevicePointer((void **)&s.d_trh, s.h_tr, 0), false);
    s.tr_cap = want;
  }
  return true;
}

/* The slot's gathered-batch buffers (fdgpu_submit_frags_io), on first use: the pinned io_records() the gather reads
   in place, and the records' device copy. */
bool slot_io_bufs(Slot &s, const fdgpu_cfg_t &c) {
  if (s.h_io) return true;
  const uint64_t m = c.max_txn + 1;
  HIPCHK(s.h_io.alloc(io_records(m).bytes), false);
  HIPCHK(hipHostGetDevicePointer((void **)&s.d_ioh, s.h_io, 0), false);
  HIPCHK(s.d_fxio.alloc(m * sizeof(fdgpu_frag_ex_t)), false);
  HIPCHK(s.d_io_cnt.alloc(64), false);
  if (g_env.io_dma) {
    HIPCHK(s.d_mirror.alloc(mirror_bytes(c)), false);
    s.mirror_cap = mirror_bytes(c) - FDGPU_ARENA_SLACK - 4096;
  }
  HIPCHK(hipMemsetAsync(s.d_io_cnt, 0, 64, s.stream), false);    /* ordered before the slot's first batch */
  return true;
}

/* The slot's item_results() of max_txn + 1 items and their pinned read-back, on its first shred or PoH batch.  d_res,
   whose presence says both are there, is allocated last: a failure part-way is retried by the next batch. */
bool slot_res_bufs(Slot &s, const fdgpu_cfg_t &c) {
  if (s.d_res) return true;
  HIPCHK(s.h_res.alloc(item_results(c.max_txn + 1).bytes), false);
  HIPCHK(s.d_res.alloc(item_results(c.max_txn + 1).bytes), false);
  return true;
}

/* (Re)size the per-lane workspace to cover n_sig signatures. */
int ensure_ws(fdgpu_engine *e, uint64_t n_sig) {
  if (n_sig <= e->ws_sig && e->d_ws) return FDGPU_OK;
  e->ws_bytes = fdgpu_ws_bytes(n_sig ? n_sig : 1);
  if (e->d_ws.alloc(e->ws_bytes) != hipSuccess) {
    set_err("workspace alloc (%zu bytes)", e->ws_bytes); e->ws_sig = 0; return FDGPU_ERR_DEVICE;
  }
  e->ws_sig = n_sig ? n_sig : 1;
  return FDGPU_OK;
}

/* the engine's registration covering [p, p + sz), or null */
const fdgpu_engine::Reg *region_of(const fdgpu_engine *e, uintptr_t p, uint64_t sz) {
  for (const auto &r : e->regions)
    if (p >= r.base && p + sz <= r.end) return &r;
  return nullptr;
}

uint32_t kflags(const fdgpu_engine_t *e) {
  return ((e->cfg.flags & FDGPU_FLAG_REF_MAPPING) ? FDGPU_FLAG_REF_MAP : 0u) |
         ((e->cfg.flags & FDGPU_FLAG_SPREAD) ? FDGPU_FLAG_KSPREAD : 0u) |
         ((e->cfg.flags & FDGPU_FLAG_FULL_PATH) ? FDGPU_FLAG_KFULL : 0u) |
         ((e->cfg.flags & FDGPU_FLAG_KEY_CACHE) ? FDGPU_FLAG_KCACHE : 0u) |
         ((e->cfg.flags & FDGPU_FLAG_PAIR) && !(e->cfg.flags & FDGPU_FLAG_KEY_CACHE) ? FDGPU_FLAG_KPAIR : 0u);
}

uint32_t ring_kflags(fdgpu_engine_t *e, Slot *s, uint64_t n_sig) {
  uint32_t f = kflags(e);
  const uint64_t auto_flags = e->cfg.flags & (FDGPU_FLAG_PAIR_AUTO | FDGPU_FLAG_SPREAD_AUTO);
  st_rlx(s->k_sigs, n_sig);
  if (auto_flags && !(f & FDGPU_FLAG_KCACHE)) {
    uint64_t load = n_sig, lanes = 0;
    if (!g_env.auto_device_scope) {
      running_load(e, s, load, lanes);
    } else {
      std::lock_guard<std::mutex> dk(g_dev_mu);
      for (const fdgpu_engine_t *o : g_dev_eng[e->device]) running_load(o, s, load, lanes);
    }
    if ((auto_flags & FDGPU_FLAG_PAIR_AUTO) && load <= FDGPU_PAIR_AUTO_SIGS) f |= FDGPU_FLAG_KPAIR;
    lanes += (f & FDGPU_FLAG_KPAIR) ? 2 * n_sig : n_sig;
    if ((auto_flags & FDGPU_FLAG_SPREAD_AUTO) && lanes <= FDGPU_SPREAD_AUTO_LANES) f |= FDGPU_FLAG_KSPREAD;
  }
  st_rlx(s->k_lanes, (f & FDGPU_FLAG_KPAIR) ? 2 * n_sig : n_sig);
  return f;
}

/* ws: a workspace for n_sig signatures, or NULL for the engine's compute workspace (grown on demand; callers on other
   streams synchronise first).  flags: ~0u for kflags(e). */
int enqueue_verify(fdgpu_engine_t *e, const uint8_t *d_arena, const fdgpu_sig_desc_t *d_sigs, const uint32_t *d_perm,
                   uint64_t n_sig, const fdgpu_txn_desc_t *d_txns, uint64_t n_txn, int8_t *d_sig_codes,
                   int8_t *d_txn_codes, hipStream_t st, uint32_t *ws, uint32_t flags) {
  if (flags == ~0u) flags = kflags(e);
  if (!ws && n_sig > e->ws_sig) {
    HIPCHK(hipStreamSynchronize(st), FDGPU_ERR_DEVICE);
    HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
    int rc = ensure_ws(e, n_sig);
    if (rc) return rc;
  }
  HIPCHK(fdgpu_launch_verify_sigs(d_arena, d_sigs, (uint32_t)n_sig, d_perm, e->d_btab, ws ? ws : e->d_ws.p, d_sig_codes,
                                  flags, st, nullptr, e->resident_blocks, e->kc_seed),
         FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_combine(d_txns, (uint32_t)n_txn, d_sig_codes, d_txn_codes, nullptr, st), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

}  // namespace fdgpu

extern "C" {

char const *fdgpu_last_error(void) { return g_err.c_str(); }

char const *fdgpu_build_info(void) {
  static thread_local char buf[512];
  char kb[256];
  const int kprod = fdgpu_kernel_build_info(kb, sizeof kb);
  const Env now;
  const int prod = kprod && FDGPU_COPY_THREADS_N == 4 && !now.drop_flag && !now.fail_merge;
  snprintf(buf, sizeof buf, "{%s,\"copy_threads\":%d,\"debug_drop_flag\":%d,\"debug_fail_merge\":%d,\"product\":%d}",
           kb, (int)FDGPU_COPY_THREADS_N, (int)now.drop_flag, now.fail_merge, prod);
  return buf;
}

int fdgpu_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) { (void)hipGetLastError(); return -1; }
  return n;
}

fdgpu_engine_t *fdgpu_engine_open(int device, fdgpu_cfg_t const *cfg_in) {
  fdgpu_cfg_t cfg{};
  if (cfg_in) cfg = *cfg_in;
  if (!cfg.max_txn) cfg.max_txn = 1u << 16;
  /* a parsed transaction carries at most 12 signatures (FD_TXN_ACTUAL_SIG_MAX, fd_txn.h:68); batches whose signatures
     exceed max_sig are rejected */
  if (!cfg.max_sig) cfg.max_sig = cfg.max_txn * 12;
  if (!cfg.max_arena) cfg.max_arena = cfg.max_txn * 1232ull;
  if (!cfg.ring_depth) cfg.ring_depth = 2;
  if (cfg.max_arena > 0xFFFFFFF0ull || cfg.max_sig > 0xFFFFFFF0ull || cfg.max_txn > 0xFFFFFFF0ull) {
    set_err("batch limits exceed 32-bit offsets");
    return nullptr;
  }
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev), nullptr);
  if (device < 0 || device >= ndev) { set_err("device %d not present (%d devices)", device, ndev); return nullptr; }
  HIPCHK(hipSetDevice(device), nullptr);
  fdgpu_engine *e = new fdgpu_engine();
  e->device = device;
  e->cfg = cfg;
  auto fail = [&]() -> fdgpu_engine_t * { fdgpu_engine_close(e); return nullptr; };
  if (hipStreamCreateWithFlags(&e->compute, hipStreamNonBlocking) != hipSuccess) { set_err("stream"); return fail(); }
  if (!(e->d_btab = btab_acquire(device, e->compute))) return fail();
  int bpcu = 0;
  hipDeviceProp_t prop;
  if (fdgpu_verify_occupancy(&bpcu) != hipSuccess || bpcu < 1) bpcu = 1;
  /* the comb build and the occupancy query loaded their units' kernels; the ingest unit's too, before the first batch */
  if (fdgpu_ingest_load() != hipSuccess) { set_err("ingest kernels"); return fail(); }
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { set_err("props"); return fail(); }
  e->resident_blocks = (uint32_t)(bpcu * prop.multiProcessorCount);
  {
    std::random_device rd;                     /* per-engine key-cache seed: crafted keys cannot target it */
    e->kc_seed = (((uint64_t)rd() << 32) | rd()) | 1u;
  }
  e->slots.resize(cfg.ring_depth);
  for (auto &s : e->slots) if (!slot_alloc(s, cfg)) return fail();
  if (hipStreamSynchronize(e->compute) != hipSuccess) { set_err("btab init failed"); return fail(); }
  const Env now;
  e->drop_flag = now.drop_flag;
  e->fail_merge_at = (uint32_t)now.fail_merge;
  /* completion words: probe that a stream write reaches pinned host memory (Env::poll_event keeps hipEventQuery
     polling) */
  {
    Slot &s0 = e->slots[0];
    if (!now.poll_event && hipStreamWriteValue32(s0.stream, s0.d_flag, 0x5a5a5a5au, 0) == hipSuccess &&
        hipStreamSynchronize(s0.stream) == hipSuccess)
      e->flag_poll = __atomic_load_n(s0.h_flag.p, __ATOMIC_ACQUIRE) == 0x5a5a5a5au;
    (void)hipGetLastError();
    *s0.h_flag = 0;
  }
  if (cfg.flags & FDGPU_FLAG_MERGE) {
    /* two merge streams (a merged verify's tail overlaps the next one's start); a table is reused only after 2 x
       ring_depth + 2 launches on its stream, by when the launch that read it has finished (every launch in flight
       holds a batch not yet complete, so at most ring_depth are) */
    e->merge_tabs = 2 * cfg.ring_depth + 2;
    e->merges.resize(now.merge_streams);
    for (auto &m : e->merges) {
      if (hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking) != hipSuccess ||
          m.h_flag.alloc(64) != hipSuccess ||
          hipHostGetDevicePointer((void **)&m.d_flag, m.h_flag, 0) != hipSuccess ||
          m.h_tab.alloc((size_t)e->merge_tabs * cfg.ring_depth * sizeof(fdgpu_mbatch_t)) != hipSuccess ||
          hipHostGetDevicePointer((void **)&m.d_tab, m.h_tab, 0) != hipSuccess) {
        set_err("merge stream");
        return fail();
      }
      *m.h_flag = 0;
      m.ev.resize(e->merge_tabs);
      for (auto &ev : m.ev)
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { set_err("merge event"); return fail(); }
    }
    e->pending.reserve(cfg.ring_depth);
  }
  {
    std::lock_guard<std::mutex> dk(g_dev_mu);
    g_dev_eng[device].push_back(e);
  }
  return e;
}

void fdgpu_engine_close(fdgpu_engine_t *e) {
  if (!e) return;
  {
    std::lock_guard<std::mutex> dk(g_dev_mu);                /* no other engine reads its slots from here on */
    auto &v = g_dev_eng[e->device];
    v.erase(std::remove(v.begin(), v.end(), e), v.end());
  }
  if (g_env.submit_prof) submit_prof_report();
  (void)hipSetDevice(e->device);
  if (e->compute) (void)hipStreamSynchronize(e->compute);
  for (auto &m : e->merges) if (m.stream) (void)hipStreamSynchronize(m.stream);
  for (auto &s : e->slots) { if (s.stream) (void)hipStreamSynchronize(s.stream); slot_free(s); }
  for (auto b : e->big) if (b) { (void)hipStreamSynchronize(b); (void)hipStreamDestroy(b); }
  for (auto &m : e->merges) {
    for (auto ev : m.ev) if (ev) (void)hipEventDestroy(ev);
    if (m.stream) (void)hipStreamDestroy(m.stream);
  }
  for (auto &r : e->regions) region_release(e->device, r.base);
  for (auto st : e->batch_streams) (void)hipStreamSynchronize(st);   /* btab is read there */
  if (e->d_btab) btab_release(e->device, e->d_btab);
  e->d_ws.reset();
  e->d_scratch_codes.reset();
  if (e->compute) (void)hipStreamDestroy(e->compute);
  delete e;
}

int fdgpu_engine_reserve(fdgpu_engine_t *e, uint64_t n_sig) {
  if (!e) return FDGPU_ERR_INVAL;
  if (!n_sig) n_sig = e->cfg.max_sig;
  if (n_sig > e->cfg.max_sig) { set_err("reserve beyond max_sig"); return FDGPU_ERR_INVAL; }
  std::lock_guard<std::mutex> lk(e->ring_mu);
  for (auto &s : e->slots) if (s.ticket >= 0 || s.staged) { set_err("a slot holds a batch"); return FDGPU_ERR_FULL; }
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  const uint64_t res = io_results(e->cfg.max_txn).bytes;
  for (auto &s : e->slots)
    if (!slot_ws(s, n_sig) || !slot_frag_bufs(s, e->cfg, res) || !slot_io_bufs(s, e->cfg)) return FDGPU_ERR_DEVICE;
  return FDGPU_OK;
}

int fdgpu_engine_info(fdgpu_engine_t *e, uint32_t *grid_blocks, uint32_t *block_threads, uint64_t *ws_bytes) {
  if (!e) return FDGPU_ERR_INVAL;
  if (grid_blocks) *grid_blocks = e->resident_blocks;
  if (block_threads) *block_threads = FDGPU_BLOCK;
  if (ws_bytes) *ws_bytes = e->ws_bytes;
  return FDGPU_OK;
}

int fdgpu_sync(fdgpu_engine_t *e) {
  if (!e) return FDGPU_ERR_INVAL;
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
  for (auto &s : e->slots) HIPCHK(hipStreamSynchronize(s.stream), FDGPU_ERR_DEVICE);
  for (auto st : e->batch_streams) HIPCHK(hipStreamSynchronize(st), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

int fdgpu_host_register(fdgpu_engine_t *e, void *p, uint64_t sz) {
  if (!e || !p || !sz) { set_err("null argument"); return FDGPU_ERR_INVAL; }
  const uintptr_t a = (uintptr_t)p & ~(uintptr_t)4095, b = ((uintptr_t)p + sz + 4095) & ~(uintptr_t)4095;
  std::lock_guard<std::mutex> lk(e->ring_mu);
  std::lock_guard<std::mutex> rk(g_reg_mu);
  /* a range inside a region already pinned (by any engine) shares it; a range that only partly overlaps one cannot be
     pinned */
  auto it = g_regions.upper_bound(a);
  uintptr_t base = 0, end = 0, dbase = 0;
  if (it != g_regions.begin()) {
    auto pv = std::prev(it);
    if (pv->first <= a && pv->second.end >= b) {
      base = pv->first; end = pv->second.end; dbase = pv->second.dbase; pv->second.refs++;
    } else if (pv->second.end > a) {
      set_err("range partly overlaps a registered region");
      return FDGPU_ERR_INVAL;
    }
  }
  if (!base) {
    if (it != g_regions.end() && it->first < b) { set_err("range partly overlaps a registered region"); return FDGPU_ERR_INVAL; }
    HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
    HIPCHK(hipHostRegister((void *)a, b - a, hipHostRegisterPortable | hipHostRegisterMapped), FDGPU_ERR_DEVICE);
    void *dp = nullptr;
    if (hipHostGetDevicePointer(&dp, (void *)a, 0) != hipSuccess || !dp) {
      (void)hipGetLastError();
      (void)hipHostUnregister((void *)a);
      set_err("registered region has no device address");
      return FDGPU_ERR_DEVICE;
    }
    g_regions[a] = {b, 1, (uintptr_t)dp};
    base = a; end = b; dbase = (uintptr_t)dp;
  }
  e->regions.push_back({a, base, end, dbase});
  return FDGPU_OK;
}

int fdgpu_host_unregister(fdgpu_engine_t *e, void *p) {
  if (!e || !p) return FDGPU_ERR_INVAL;
  const uintptr_t a = (uintptr_t)p & ~(uintptr_t)4095;
  std::lock_guard<std::mutex> lk(e->ring_mu);
  for (size_t i = e->regions.size(); i-- > 0;) {            /* the latest registration of this range */
    if (e->regions[i].user != a) continue;
    for (auto &sl : e->slots) if (sl.stream) (void)hipStreamSynchronize(sl.stream);   /* no DMA still reads it */
    region_release(e->device, e->regions[i].base);
    e->regions.erase(e->regions.begin() + (long)i);
    return FDGPU_OK;
  }
  set_err("region not registered with this engine");
  return FDGPU_ERR_INVAL;
}

}  // extern "C"
