/* fdgpu_ring.cpp -- the engine's ring API: a batch is staged into a free slot, queued on the slot's stream, published
   under a ticket, polled and released (fdgpu_submit, fdgpu_stage_*, fdgpu_poll*, fdgpu_release), and
   fdgpu_verify_device on the compute stream. */
#include <algorithm>

#include "fdgpu_engine.h"

using namespace fdgpu;

namespace {

/* A ring batch of at least this many signatures fills every resident lane of the chip (256 CUs x 4 SIMDs x 2 waves x
   64 = 131,072) on its own.  Its verify runs on one of the engine's two big-batch streams, in turn, after its uploads
   (an event wait), and its read-back waits for it: at most two such verifies overlap (the next one's waves fill the
   tail the previous one leaves, as the device-resident line's two queues do), and the next slots' uploads run under
   them.  On their own slot streams three 1 M batches ran in lockstep -- three uploads at once with the GPU idle, then
   three verifies at once -- 11.6-12.0 ms a batch from a registered arena against 10.3 staged (rocprofv3 with
   --memory-copy-trace, profiles/r05/host_fed_lockstep.md).  Env::big_streams turns it off. */
constexpr uint64_t FDGPU_BIG_SIGS = 262144;

/* arenas of at least this many bytes are staged by FDGPU_COPY_THREADS threads */
constexpr uint64_t FDGPU_COPY_SPLIT_MIN = 4ull << 20;

/* the last FDGPU_ST_RING fdgpu_submit calls of the process: {staging copy, descriptor expansion, enqueue} ns
   (fdgpu_debug_submit_times).  Each call writes the entry its fetch_add drew; the words are relaxed atomics, so
   concurrent submitters and a reader never race (a reader may see a triple that a writer is mid-way through, which is
   a diagnostic's tolerance) */
constexpr uint64_t FDGPU_ST_RING = 8192;
std::atomic<uint64_t> g_st[FDGPU_ST_RING][3];
std::atomic<uint64_t> g_st_n{0};

}  // namespace

namespace fdgpu {

/* A free slot of the ring (ring_mu held), the engine's device made the thread's current one: FDGPU_OK and *s, or the
   error with its text set. */
int take_slot(fdgpu_engine_t *e, Slot **s) {
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  for (auto &c : e->slots) if (c.ticket < 0 && !c.staged) { *s = &c; return FDGPU_OK; }
  set_err("all ring slots hold unpolled batches");
  return FDGPU_ERR_FULL;
}

/* The end of a batch's work on its stream: the next sequence number, the completion word the stream writes after
   everything before it (unless the engine polls events, or the test hook drops it), the done event. */
int slot_signal(fdgpu_engine_t *e, Slot *s) {
  __atomic_store_n(&s->flag_seq, s->flag_seq + 1, __ATOMIC_RELEASE);
  if (e->flag_poll && !e->drop_flag) HIPCHK(hipStreamWriteValue32(s->stream, s->d_flag, s->flag_seq, 0), FDGPU_ERR_DEVICE);
  HIPCHK(hipEventRecord(s->done, s->stream), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

/* Publish the batch queued on slot s (ring_mu held): signal its end -- unless the caller has deferred that
   (signal_deferred: its verify waits to be merged, io_tail signals behind it) -- and hand out its ticket.  Returns
   the ticket, or the signal's error with the slot left free. */
int64_t slot_publish(fdgpu_engine_t *e, Slot *s, Batch kind, uint64_t txn_cnt, uint64_t tr_sz, uint64_t tr_base,
                     bool signal_deferred) {
  if (!signal_deferred) {
    const int rc = slot_signal(e, s);
    if (rc) return rc;
  }
  s->staged = false;
  st_rlx(s->held, false);
  st_rlx(s->polls, 0u);
  s->kind = kind;
  s->tr_sz = tr_sz;
  s->tr_base = tr_base;
  s->txn_cnt = txn_cnt;
  st_rlx(s->ticket, e->next_ticket++);
  return s->ticket;
}

/* Copy a caller's arena into the slot's pinned buffer.  Large arenas are split over FDGPU_COPY_THREADS host threads;
   each queues its part's upload on the slot stream as soon as its memcpy is done, so the PCIe copy runs under the
   rest of the staging (one core's memcpy bandwidth, ~15 GB/s, otherwise bounds submit()).  Returns the bytes already
   queued for upload, or UINT64_MAX on a HIP error.  An arena that expand() later rejects leaves the slot free; its
   stale upload is overwritten by the next batch's copies, which are ordered after it on the same stream. */
static uint64_t stage_arena(fdgpu_engine_t *e, Slot *s, uint8_t const *arena, uint64_t sz) {
  if (sz < FDGPU_COPY_SPLIT_MIN) {
    memcpy(s->h_arena, arena, sz);
    return 0;
  }
  const uint64_t part = ((sz + FDGPU_COPY_THREADS - 1) / FDGPU_COPY_THREADS + 63) & ~63ull;
  const uint64_t chunk = g_env.copy_chunk;
  int err[FDGPU_COPY_THREADS] = {};
  std::vector<std::function<void()>> fns;
  for (unsigned i = 0; i < FDGPU_COPY_THREADS; i++)
    fns.push_back([&, i]() {
      const uint64_t off = (uint64_t)i * part;
      if (off >= sz) return;
      const uint64_t n = sz - off < part ? sz - off : part;
      if (hipSetDevice(e->device) != hipSuccess) { err[i] = 1; return; }
      /* in Env::copy_chunk pieces, each queued for upload as soon as it is copied: the DMA starts ~1 ms into the
         staging instead of after it (a 1 M batch's 364 MB: its uploads then end ~3 ms sooner) */
      for (uint64_t c = 0; c < n; c += chunk) {
        const uint64_t m = n - c < chunk ? n - c : chunk;
        memcpy(s->h_arena + off + c, arena + off + c, m);
        if (hipMemcpyAsync(s->d_arena + off + c, s->h_arena + off + c, m, hipMemcpyHostToDevice, s->stream) !=
            hipSuccess) { err[i] = 1; return; }
      }
    });
  copy_run(fns);
  for (unsigned i = 0; i < FDGPU_COPY_THREADS; i++)
    if (err[i]) { set_err("staging upload failed"); return UINT64_MAX; }
  return sz;
}

/* Queue the upload of a frag, shred or PoH batch's whole arena on the slot's stream: one copy straight from the
   caller's memory where that lies in a registered region (its bytes must stay unchanged until the batch is polled),
   else staged through the slot's pinned buffer.  The slack past the arena needs no zeroing: every device reader of
   these batches masks the bytes past its item in registers (fdt_reader, msg_block, fdgpu_sha256.h), only their
   presence (FDGPU_ARENA_SLACK allocated) matters. */
int slot_upload(fdgpu_engine_t *e, Slot *s, uint8_t const *arena, uint64_t arena_sz) {
  if (region_of(e, (uintptr_t)arena, arena_sz)) {
    if (arena_sz) HIPCHK(hipMemcpyAsync(s->d_arena, arena, arena_sz, hipMemcpyHostToDevice, s->stream), FDGPU_ERR_DEVICE);
    return FDGPU_OK;
  }
  const uint64_t up = stage_arena(e, s, arena, arena_sz);
  if (up == UINT64_MAX) return FDGPU_ERR_DEVICE;
  if (arena_sz > up)
    HIPCHK(hipMemcpyAsync(s->d_arena + up, s->h_arena + up, arena_sz - up, hipMemcpyHostToDevice, s->stream),
           FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

}  // namespace fdgpu

namespace {

/* Enqueue the batch already in slot s's pinned arena (arena_sz bytes). */
/* `uploaded` = bytes of the arena whose host->device copy is already queued on the slot's stream (fdgpu_submit
   overlaps its staging memcpy with the copy) */
/* src != NULL: the arena lies in a registered host region and is uploaded straight from there (no staging copy); its
   bytes must stay unchanged until the batch is polled. */
int64_t submit_slot(fdgpu_engine_t *e, Slot *s, uint64_t arena_sz, fdgpu_txn_t const *txns, uint64_t txn_cnt,
                    uint64_t uploaded = 0, const uint8_t *src = nullptr, uint64_t t_stage = 0) {
  uint32_t *perm = bucket(e) ? s->h_perm.p : nullptr;
  /* a registered arena's DMA is queued first, so it runs under the descriptor expansion (an arena expand() rejects
     leaves the slot free; the next batch's copies, later on the same stream, overwrite it) */
  if (src && arena_sz) HIPCHK(hipMemcpyAsync(s->d_arena, src, arena_sz, hipMemcpyHostToDevice, s->stream), FDGPU_ERR_DEVICE);
  const uint64_t t0 = sp_now();
  const int64_t ns = expand_par(arena_sz, txns, txn_cnt, e->cfg.max_sig, s->h_sigs, s->h_txns, perm);
  if (ns < 0) return FDGPU_ERR_INVAL;
  const uint64_t t1 = sp_now();
  struct Rec {                                  /* the call's times into the ring, on every return */
    uint64_t st, t0, t1;
    ~Rec() {
      const uint64_t k = g_st_n.fetch_add(1, std::memory_order_relaxed) % FDGPU_ST_RING;
      g_st[k][0].store(st, std::memory_order_relaxed);
      g_st[k][1].store(t1 - t0, std::memory_order_relaxed);
      g_st[k][2].store(sp_now() - t1, std::memory_order_relaxed);
    }
  } rec{t_stage, t0, t1};
  if (!slot_ws(*s, (uint64_t)ns)) return FDGPU_ERR_DEVICE;
  if (src) {
    /* the slack past a registered arena is left as it is: the SHA block loads mask every byte past the message
       (msg_block), so only its presence matters.  Zeroing it on the device cost a kernel (a fill, or the blit of a
       small copy) queued behind the upload, which waits for a CU slot the running verify holds -- the batch's
       descriptor copies and verify waited behind it, ~7 ms a 1 M batch (profiles/r05/host_fed/registered_slack.md) */
  } else {
    memset(s->h_arena + arena_sz, 0, FDGPU_ARENA_SLACK);
    const size_t asz = arena_sz + FDGPU_ARENA_SLACK - uploaded;
    HIPCHK(hipMemcpyAsync(s->d_arena + uploaded, s->h_arena + uploaded, asz, hipMemcpyHostToDevice, s->stream),
           FDGPU_ERR_DEVICE);
  }
  if (ns) HIPCHK(hipMemcpyAsync(s->d_sigs, s->h_sigs, (size_t)ns * sizeof(fdgpu_sig_desc_t), hipMemcpyHostToDevice, s->stream), FDGPU_ERR_DEVICE);
  if (ns && perm) HIPCHK(hipMemcpyAsync(s->d_perm, perm, (size_t)ns * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream), FDGPU_ERR_DEVICE);
  if (txn_cnt) HIPCHK(hipMemcpyAsync(s->d_txns, s->h_txns, txn_cnt * sizeof(fdgpu_txn_desc_t), hipMemcpyHostToDevice, s->stream), FDGPU_ERR_DEVICE);
  /* copies, kernels and the code read-back of a slot run in order on the slot's own stream with the slot's own
     workspace, so the ring's batches overlap each other on the GPU (a 64K-signature batch fills only half of the
     resident wave slots) */
  hipStream_t vs = s->stream;
  if ((uint64_t)ns >= FDGPU_BIG_SIGS && g_env.big_streams) {
    for (auto &b : e->big)
      if (!b) HIPCHK(hipStreamCreateWithFlags(&b, hipStreamNonBlocking), FDGPU_ERR_DEVICE);
    vs = e->big[e->big_rr++ & 1u];
    HIPCHK(hipEventRecord(s->h2d_done, s->stream), FDGPU_ERR_DEVICE);
    HIPCHK(hipStreamWaitEvent(vs, s->h2d_done, 0), FDGPU_ERR_DEVICE);
  }
  int rc = enqueue_verify(e, s->d_arena, s->d_sigs, perm ? s->d_perm.p : nullptr, (uint64_t)ns, s->d_txns, txn_cnt,
                          s->d_sig_codes, s->d_txn_codes, vs, s->d_ws, ring_kflags(e, s, (uint64_t)ns));
  if (rc) return rc;
  if (vs != s->stream) {
    HIPCHK(hipEventRecord(s->comp_done, vs), FDGPU_ERR_DEVICE);
    HIPCHK(hipStreamWaitEvent(s->stream, s->comp_done, 0), FDGPU_ERR_DEVICE);
  }
  if (txn_cnt) HIPCHK(hipMemcpyAsync(s->h_codes, s->d_txn_codes, txn_cnt, hipMemcpyDeviceToHost, s->stream), FDGPU_ERR_DEVICE);
  return slot_publish(e, s, Batch::Ring, txn_cnt, 0, 0);
}

}  // namespace

namespace fdgpu {

int poll_slot(fdgpu_engine_t *e, int64_t ticket, int8_t *txn_codes, int blocking, bool keep, uint8_t *trailers,
              uint64_t *tags, uint16_t *out_szs, uint8_t *items, uint32_t *rep, uint64_t *lanes) {
  if (!e) return FDGPU_ERR_INVAL;
  /* a batch still on the device is answered without the ring lock: the caller owns its ticket's slot until a poll
     returns it done, so the slot's ticket and completion word are stable here; the runtime check below (every 256th
     poll) and everything else take the lock */
  bool counted = false;                        /* this poll already counted in the slot's polls */
  if (!blocking && e->flag_poll && e->merges.empty() && ticket >= 0)
    for (auto &c : e->slots)
      if (__atomic_load_n(&c.ticket, __ATOMIC_RELAXED) == ticket) {
        if (!__atomic_load_n(&c.held, __ATOMIC_RELAXED) &&
            __atomic_load_n(c.h_flag.p, __ATOMIC_ACQUIRE) != __atomic_load_n(&c.flag_seq, __ATOMIC_RELAXED)) {
          counted = true;
          if ((__atomic_add_fetch(&c.polls, 1u, __ATOMIC_RELAXED) & 255u) != 0) return FDGPU_PENDING;
        }
        break;
      }
  std::unique_lock<std::mutex> lk(e->ring_mu);
  Slot *s = nullptr;
  for (auto &c : e->slots) if (c.ticket == ticket && ticket >= 0 && !c.held) { s = &c; break; }
  if (!s) { set_err("unknown ticket %lld", (long long)ticket); return FDGPU_ERR_TICKET; }
  if (s->failed) {                             /* its merged verify was never queued (merge_kick) */
    s->failed = false;
    st_rlx(s->ticket, (int64_t)-1);
    set_err("ticket %lld: its verify could not be queued", (long long)ticket);
    return FDGPU_ERR_DEVICE;
  }
  if (!e->pending.empty()) {                   /* FDGPU_FLAG_MERGE: verifies waiting for a merge stream */
    HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
    const int rc = merge_kick(e, blocking && s->vpending);
    if (rc) return rc;
    if (s->vpending) return FDGPU_PENDING;     /* non-blocking: not even launched */
  }
  if (blocking) {
    HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
    lk.unlock();                               /* the slot is this caller's until it is polled */
    HIPCHK(hipEventSynchronize(s->done), FDGPU_ERR_DEVICE);
    lk.lock();
  } else if (e->flag_poll) {
    /* the stream wrote flag_seq after the codes' read-back completed.  A stream that failed never writes it, so an
       unanswered poll asks the runtime now and then -- every 256th poll once 1 ms has passed since the last question
       (runtime queries from several tile threads contend): an error ends the wait (the tile stops instead of polling
       forever), a completed event means the batch is done. */
    if (__atomic_load_n(s->h_flag.p, __ATOMIC_ACQUIRE) != s->flag_seq) {
      if (!counted && (__atomic_add_fetch(&s->polls, 1u, __ATOMIC_RELAXED) & 255u) != 0) return FDGPU_PENDING;
      const uint64_t now = sp_now();
      if (now - s->last_query < 1000000ull) return FDGPU_PENDING;
      s->last_query = now;
      HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
      const hipError_t q = hipEventQuery(s->done);
      if (q == hipErrorNotReady) return FDGPU_PENDING;
      HIPCHK(q, FDGPU_ERR_DEVICE);
    }
  } else {
    HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
    hipError_t q = hipEventQuery(s->done);
    if (q == hipErrorNotReady) return FDGPU_PENDING;
    HIPCHK(q, FDGPU_ERR_DEVICE);
  }
  const uint64_t n = s->txn_cnt;
  switch (s->kind) {
    case Batch::Ring:
      if (txn_codes && n) memcpy(txn_codes, s->h_codes, n);
      break;
    case Batch::Frag:
      if (txn_codes && n) memcpy(txn_codes, s->h_tr, n);
      if (trailers && s->tr_sz) memcpy(trailers, s->h_tr + s->tr_base, s->tr_sz);
      break;
    case Batch::FragIo: {
      const IoResults r = io_results(n);
      if (txn_codes && n) memcpy(txn_codes, s->h_tr, n);
      if (tags && n) memcpy(tags, s->h_tr + r.tags, n * 8);
      if (out_szs && n) memcpy(out_szs, s->h_tr + r.sizes, n * 2);
      break;
    }
    case Batch::Shred:
    case Batch::Poh:
      if (txn_codes && n) memcpy(txn_codes, s->h_res, n);
      if (items && n) memcpy(items, s->h_res + item_results(n).items, n * 32);
      break;
    case Batch::Precompile:
    case Batch::Secp256k1:
      if (txn_codes && n) memcpy(txn_codes, s->h_res, n);
      if (items && n) memcpy(items, s->h_res + item_results(n, 16).items, n * 16);
      break;
    case Batch::ShredSets: {
      const SetResults r = set_results(n);
      if (txn_codes && n) memcpy(txn_codes, s->h_sres, n);
      if (items && n) memcpy(items, s->h_sres + r.roots, n * 32);
      if (rep && n) memcpy(rep, s->h_sres + r.rep, n * 4);
      if (lanes) { uint32_t l = 0; if (n) memcpy(&l, s->h_sres + r.lanes, 4); *lanes = l; }
      break;
    }
  }
  if (keep) st_rlx(s->held, true);
  else st_rlx(s->ticket, (int64_t)-1);
  return FDGPU_OK;
}

}  // namespace fdgpu

extern "C" {

int64_t fdgpu_submit(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_txn_t const *txns,
                     uint64_t txn_cnt) {
  if (!e || (!arena && arena_sz) || (!txns && txn_cnt)) { set_err("null argument"); return FDGPU_ERR_INVAL; }
  if (arena_sz > e->cfg.max_arena || txn_cnt > e->cfg.max_txn) { set_err("batch exceeds engine limits"); return FDGPU_ERR_INVAL; }
  std::lock_guard<std::mutex> lk(e->ring_mu);
  Slot *s = nullptr;
  if (const int rc = take_slot(e, &s)) return rc;
  /* not slot_upload: a staged arena's last copy carries the zeroed slack and is queued after the expansion, under
     which the parts already queued run (submit_slot) */
  if (region_of(e, (uintptr_t)arena, arena_sz)) return submit_slot(e, s, arena_sz, txns, txn_cnt, 0, arena);
  /* the slot's previous batch was polled, so its copies are complete */
  const uint64_t ts = sp_now();
  const uint64_t up = stage_arena(e, s, arena, arena_sz);
  if (up == UINT64_MAX) return FDGPU_ERR_DEVICE;
  return submit_slot(e, s, arena_sz, txns, txn_cnt, up, nullptr, sp_now() - ts);
}

uint8_t *fdgpu_stage_acquire(fdgpu_engine_t *e, uint64_t *cap) {
  if (!e) return nullptr;
  std::lock_guard<std::mutex> lk(e->ring_mu);
  for (auto &c : e->slots) if (c.staged) { set_err("a slot is already staged"); return nullptr; }
  Slot *s = nullptr;
  if (take_slot(e, &s)) return nullptr;
  s->staged = true;
  if (cap) *cap = e->cfg.max_arena;
  return s->h_arena;
}

int64_t fdgpu_stage_submit(fdgpu_engine_t *e, uint64_t arena_sz, fdgpu_txn_t const *txns, uint64_t txn_cnt) {
  if (!e || (!txns && txn_cnt)) { set_err("null argument"); return FDGPU_ERR_INVAL; }
  std::lock_guard<std::mutex> lk(e->ring_mu);
  Slot *s = nullptr;
  for (auto &c : e->slots) if (c.staged) { s = &c; break; }
  if (!s) { set_err("no staged slot"); return FDGPU_ERR_INVAL; }
  if (arena_sz > e->cfg.max_arena || txn_cnt > e->cfg.max_txn) { set_err("batch exceeds engine limits"); return FDGPU_ERR_INVAL; }
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  return submit_slot(e, s, arena_sz, txns, txn_cnt);
}

int fdgpu_stage_cancel(fdgpu_engine_t *e) {
  if (!e) return FDGPU_ERR_INVAL;
  std::lock_guard<std::mutex> lk(e->ring_mu);
  for (auto &c : e->slots) if (c.staged) { c.staged = false; return FDGPU_OK; }
  return FDGPU_ERR_INVAL;
}

int fdgpu_poll(fdgpu_engine_t *e, int64_t ticket, int8_t *txn_codes, int blocking) {
  return poll_slot(e, ticket, txn_codes, blocking, false);
}

int fdgpu_poll_keep(fdgpu_engine_t *e, int64_t ticket, int8_t *txn_codes, int blocking) {
  return poll_slot(e, ticket, txn_codes, blocking, true);
}

int fdgpu_poll_frags(fdgpu_engine_t *e, int64_t ticket, int8_t *codes, uint8_t *trailers, int blocking) {
  return poll_slot(e, ticket, codes, blocking, false, trailers);
}

int fdgpu_poll_frags_io(fdgpu_engine_t *e, int64_t ticket, int8_t *codes, uint64_t *tags, uint16_t *out_szs,
                        int blocking) {
  return poll_slot(e, ticket, codes, blocking, false, nullptr, tags, out_szs);
}

int fdgpu_release(fdgpu_engine_t *e, int64_t ticket) {
  if (!e) return FDGPU_ERR_INVAL;
  std::lock_guard<std::mutex> lk(e->ring_mu);
  for (auto &c : e->slots)
    if (c.ticket == ticket && ticket >= 0 && c.held) { st_rlx(c.held, false); st_rlx(c.ticket, (int64_t)-1); return FDGPU_OK; }
  set_err("ticket %lld not held", (long long)ticket);
  return FDGPU_ERR_TICKET;
}

int fdgpu_verify_device(fdgpu_engine_t *e, void const *d_arena, void const *d_sig_desc, uint64_t sig_cnt,
                        void const *d_txn_desc, uint64_t txn_cnt, int8_t *d_sig_codes, int8_t *d_txn_codes,
                        void *hip_stream) {
  if (!e || sig_cnt > 0xFFFFFFF0ull || txn_cnt > 0xFFFFFFF0ull) return FDGPU_ERR_INVAL;
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : e->compute;
  if (!d_sig_codes) {
    if (e->scratch_cap < sig_cnt + 16) {
      if (e->d_scratch_codes) HIPCHK(hipStreamSynchronize(st), FDGPU_ERR_DEVICE);
      HIPCHK(e->d_scratch_codes.alloc(sig_cnt + 16), FDGPU_ERR_DEVICE);
      e->scratch_cap = sig_cnt + 16;
    }
    d_sig_codes = e->d_scratch_codes;
  }
  return enqueue_verify(e, (const uint8_t *)d_arena, (const fdgpu_sig_desc_t *)d_sig_desc, nullptr, sig_cnt,
                        (const fdgpu_txn_desc_t *)d_txn_desc, txn_cnt, d_sig_codes, d_txn_codes, st);
}

uint64_t fdgpu_debug_submit_times(uint64_t *out, uint64_t max) {
  const uint64_t n = std::min<uint64_t>(g_st_n.load(), FDGPU_ST_RING), m = std::min(n, max);
  const uint64_t end = g_st_n.load();
  for (uint64_t i = 0; i < m; i++) {
    const uint64_t k = (end - m + i) % FDGPU_ST_RING;
    for (int j = 0; j < 3; j++) out[3 * i + j] = g_st[k][j].load(std::memory_order_relaxed);
  }
  return m;
}

double fdgpu_debug_h2d_gbps(fdgpu_engine_t *e, void const *src, uint64_t sz, int iters) {
  if (!e || !src || !sz || iters < 1 || sz > e->cfg.max_arena) { set_err("bad argument"); return -1.0; }
  std::lock_guard<std::mutex> lk(e->ring_mu);
  Slot *s = nullptr;
  if (take_slot(e, &s)) return -1.0;
  Events ev;
  if (!ev.create(2)) { (void)hipGetLastError(); set_err("event"); return -1.0; }
  const hipEvent_t a = ev[0], b = ev[1];
  double gbps = -1.0;
  float ms = 0.f;
  if (hipMemcpyAsync(s->d_arena, src, sz, hipMemcpyHostToDevice, s->stream) == hipSuccess &&   /* warm */
      hipEventRecord(a, s->stream) == hipSuccess) {
    bool ok = true;
    for (int i = 0; i < iters && ok; i++)
      ok = hipMemcpyAsync(s->d_arena, src, sz, hipMemcpyHostToDevice, s->stream) == hipSuccess;
    if (ok && hipEventRecord(b, s->stream) == hipSuccess && hipEventSynchronize(b) == hipSuccess &&
        hipEventElapsedTime(&ms, a, b) == hipSuccess && ms > 0.f)
      gbps = (double)sz * iters / (ms * 1e-3) / 1e9;
  }
  (void)hipGetLastError();
  if (gbps < 0) set_err("h2d timing failed");
  return gbps;
}

}  // extern "C"
