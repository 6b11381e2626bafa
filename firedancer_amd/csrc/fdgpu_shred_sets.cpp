/* fdgpu_shred_sets.cpp -- every shred of a batch through the engine, one verify lane per FEC set
   (include/fd_shred_sets_gpu.h): the ring batch (fdgpu_submit_shred_sets / fdgpu_poll_shred_sets) and its timing
   diagnostic.  A batch is its arena uploaded as a shred batch's, then on the slot's stream set ingest (checks, SHA-256
   leaf and proof walk, roots into the arena's roots region, a state per shred) -> set dedup (one signature descriptor
   per distinct key among the shreds without a known root) -> verify -> set finish (codes, roots, representatives and
   the lane count side by side) and one read-back. */
#include "fdgpu_engine.h"
#include "fdgpu_shred.h"

using namespace fdgpu;

namespace {

/* the dedup's table for n shreds: a power of two >= 2 n words, at least 64 */
uint64_t ht_slots(uint64_t n) {
  uint64_t s = 64;
  while (s < 2 * n) s <<= 1;
  return s;
}

/* Checks every argument of a set batch as shred_args (fdgpu_shreds.cpp) does a shred batch's, and the known roots; the
   roots region lies behind the arena and its slack, inside `cap`.  0, or FDGPU_ERR_INVAL with the error text set. */
int set_args(const fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_set_shred_t const *sh, uint64_t n,
             uint64_t cap, uint64_t *roots_off) {
  if (!e || (!arena && arena_sz) || (!sh && n)) { set_err("null argument"); return FDGPU_ERR_INVAL; }
  if (n > e->cfg.max_txn || n > e->cfg.max_sig || n > 0x7FFFFFFull) { set_err("batch exceeds engine limits"); return FDGPU_ERR_INVAL; }
  for (uint64_t i = 0; i < n; i++) {
    if ((uint64_t)sh[i].off + sh[i].sz > arena_sz || (uint64_t)sh[i].pub_off + 32 > arena_sz || sh[i].sz > FDGPU_SHRED_SZ_MAX) {
      set_err("shred %llu: out of the arena, or larger than %u bytes", (unsigned long long)i, FDGPU_SHRED_SZ_MAX);
      return FDGPU_ERR_INVAL;
    }
    if (sh[i].known_off != FDGPU_SHRED_NO_ROOT && (uint64_t)sh[i].known_off + 32 > arena_sz) {
      set_err("shred %llu: its known root lies outside the arena", (unsigned long long)i);
      return FDGPU_ERR_INVAL;
    }
  }
  *roots_off = (arena_sz + FDGPU_ARENA_SLACK + 15) & ~15ull;
  if (*roots_off + 32 * n > cap) {
    set_err("arena (%llu B), slack and %llu roots exceed the arena allocation (%llu B)", (unsigned long long)arena_sz,
            (unsigned long long)n, (unsigned long long)cap);
    return FDGPU_ERR_INVAL;
  }
  return FDGPU_OK;
}

/* the slot's set-batch buffers, on its first set batch.  d_set, whose presence says all are there, is allocated last:
   a failure part-way is retried by the next batch. */
bool slot_set_bufs(Slot &s, const fdgpu_cfg_t &c) {
  if (s.d_set) return true;
  const uint64_t n = c.max_txn + 1;
  HIPCHK(s.h_set.alloc(n * sizeof(fdgpu_set_shred_t)), false);
  HIPCHK(s.d_set_state.alloc(n), false);
  HIPCHK(s.d_set_ht.alloc(ht_slots(n) * sizeof(uint32_t)), false);
  HIPCHK(s.d_set_slot.alloc(n * sizeof(uint32_t)), false);
  HIPCHK(s.d_set_cnt.alloc(64), false);
  HIPCHK(s.h_sres.alloc(set_results(n).bytes), false);
  HIPCHK(s.d_sres.alloc(set_results(n).bytes), false);
  HIPCHK(s.d_set.alloc(n * sizeof(fdgpu_set_shred_t)), false);
  return true;
}

/* the stages before the verify, queued on st: the count and the table cleared, set ingest, set dedup */
int queue_ingest(uint8_t *d_arena, const fdgpu_set_shred_t *d_set, uint64_t n, uint16_t version, uint64_t roots_off,
                 uint8_t *d_state, uint32_t *d_ht, uint64_t seed, uint32_t *d_rep, uint32_t *d_slot,
                 fdgpu_sig_desc_t *d_sigs, uint32_t *d_cnt, hipStream_t st) {
  const uint64_t slots = ht_slots(n);
  HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(uint32_t), st), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemsetAsync(d_ht, 0xff, slots * sizeof(uint32_t), st), FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_shred_set_ingest(d_arena, d_set, (uint32_t)n, version, (uint32_t)roots_off, d_state, st),
         FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_shred_set_dedup(d_arena, d_set, (uint32_t)n, (uint32_t)roots_off, d_state, d_ht, (uint32_t)slots,
                                      seed, d_rep, d_slot, d_sigs, d_cnt, st),
         FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

}  // namespace

extern "C" {

int64_t fdgpu_submit_shred_sets(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_set_shred_t const *sh,
                                uint64_t n, uint16_t expected_version) {
  if (e && arena_sz > e->cfg.max_arena) { set_err("batch exceeds engine limits"); return FDGPU_ERR_INVAL; }
  uint64_t roots_off = 0;
  const int arc = set_args(e, arena, arena_sz, sh, n, e ? e->cfg.max_arena : 0, &roots_off);
  if (arc) return arc;
  std::lock_guard<std::mutex> lk(e->ring_mu);
  Slot *s = nullptr;
  if (const int rc = take_slot(e, &s)) return rc;
  if (!n) return slot_publish(e, s, Batch::ShredSets, 0, 0, 0);
  if (!slot_set_bufs(*s, e->cfg) || !slot_ws(*s, n)) return FDGPU_ERR_DEVICE;
  if (const int rc = slot_upload(e, s, arena, arena_sz)) return rc;
  const SetResults res = set_results(n);
  uint32_t *d_rep = (uint32_t *)(s->d_sres + res.rep);
  memcpy(s->h_set, sh, n * sizeof(fdgpu_set_shred_t));
  HIPCHK(hipMemcpyAsync(s->d_set, s->h_set, n * sizeof(fdgpu_set_shred_t), hipMemcpyHostToDevice, s->stream), FDGPU_ERR_DEVICE);
  if (const int rc = queue_ingest(s->d_arena, s->d_set, n, expected_version, roots_off, s->d_set_state, s->d_set_ht,
                                  e->kc_seed, d_rep, s->d_set_slot, s->d_sigs, s->d_set_cnt, s->stream))
    return rc;
  /* n bounds the signature count (one per distinct key); the count itself stays on the device */
  HIPCHK(fdgpu_launch_verify_sigs(s->d_arena, s->d_sigs, (uint32_t)n, nullptr, e->d_btab, s->d_ws, s->d_sig_codes,
                                  ring_kflags(e, s, n), s->stream, s->d_set_cnt, e->resident_blocks, e->kc_seed),
         FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_shred_set_finish(s->d_set_state, d_rep, s->d_set_slot, (uint32_t)n, s->d_sig_codes,
                                       s->d_arena + roots_off, s->d_set_cnt, (int8_t *)s->d_sres.p, s->d_sres + res.roots,
                                       (uint32_t *)(s->d_sres + res.lanes), s->stream),
         FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpyAsync(s->h_sres, s->d_sres, res.bytes, hipMemcpyDeviceToHost, s->stream), FDGPU_ERR_DEVICE);
  return slot_publish(e, s, Batch::ShredSets, n, 0, 0);
}

int fdgpu_poll_shred_sets(fdgpu_engine_t *e, int64_t ticket, int8_t *codes, uint8_t *roots, uint32_t *rep, uint64_t *lanes,
                          int blocking) {
  return poll_slot(e, ticket, codes, blocking, false, nullptr, nullptr, nullptr, roots, rep, lanes);
}

int fdgpu_debug_shred_sets_time(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_set_shred_t const *sh,
                                uint64_t n, uint16_t expected_version, int iters, double *ingest_ms, double *verify_ms) {
  if (iters < 1 || !ingest_ms || !verify_ms) { set_err("bad argument"); return FDGPU_ERR_INVAL; }
  if (!n) { set_err("empty batch"); return FDGPU_ERR_INVAL; }
  uint64_t roots_off = 0;
  int rc = set_args(e, arena, arena_sz, sh, n, UINT32_MAX - 64ull * 1024, &roots_off);
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  DevBuf<uint8_t> d_arena, d_state;
  DevBuf<fdgpu_set_shred_t> d_set;
  DevBuf<fdgpu_sig_desc_t> d_sigs;
  DevBuf<uint32_t> d_ht, d_rep, d_slot, d_cnt;
  DevBuf<int8_t> d_sig_codes;
  /* the roots region behind the arena and its slack, zeroed with them */
  HIPCHK(dev_arena(d_arena, arena, arena_sz, roots_off + 32 * n - arena_sz, false), FDGPU_ERR_DEVICE);
  if (d_state.alloc(n) || d_set.alloc(n * sizeof(fdgpu_set_shred_t)) || d_sigs.alloc(n * sizeof(fdgpu_sig_desc_t) + 16) ||
      d_ht.alloc(ht_slots(n) * sizeof(uint32_t)) || d_rep.alloc(n * sizeof(uint32_t)) ||
      d_slot.alloc(n * sizeof(uint32_t)) || d_cnt.alloc(64) || d_sig_codes.alloc(n + 16)) {
    (void)hipGetLastError();
    set_err("alloc");
    return FDGPU_ERR_DEVICE;
  }
  HIPCHK(hipMemcpy(d_set, sh, n * sizeof(fdgpu_set_shred_t), hipMemcpyHostToDevice), FDGPU_ERR_DEVICE);
  if (n > e->ws_sig) {
    HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
    rc = ensure_ws(e, n);
    if (rc) return rc;
  }
  hipStream_t st = e->compute;
  /* the warm-up also leaves the descriptors and the count the timed verifies read */
  auto ingest = [&] {
    return !queue_ingest(d_arena, d_set, n, expected_version, roots_off, d_state, d_ht, e->kc_seed, d_rep, d_slot, d_sigs,
                         d_cnt, st);
  };
  auto verify = [&] {
    return fdgpu_launch_verify_sigs(d_arena, d_sigs, (uint32_t)n, nullptr, e->d_btab, e->d_ws, d_sig_codes, kflags(e), st,
                                    d_cnt, e->resident_blocks, e->kc_seed) == hipSuccess;
  };
  return time_two_stages(st, iters, "shred sets", [&] { return ingest() && verify(); }, ingest, verify, ingest_ms,
                         verify_ms);
}

}  // extern "C"
