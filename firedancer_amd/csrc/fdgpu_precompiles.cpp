/* fdgpu_precompiles.cpp -- a block's Ed25519 precompile instructions through the engine (include/fd_precompile_gpu.h):
   the ring batch (fdgpu_submit_precompiles / fdgpu_poll_precompiles) and the precompile diagnostics.  A batch is its
   arena uploaded as any frag batch's, then on the slot's stream ingest (parse, the walk over the record tables, one
   signature descriptor per record that resolves) -> verify -> finish (codes and infos side by side) and one
   read-back. */
#include "fdgpu_engine.h"
#include "fdgpu_precompile.h"
#include "fdt_precompile.h"

using namespace fdgpu;

static_assert(sizeof(fdgpu_precompile_info_t) == 16 && sizeof(fdgpu_precompile_walk_t) == 16 &&
              sizeof(fdgpu_precompile_t) == 12, "the kernels store these as words");

namespace fdgpu {

/* Checks every argument of a precompile batch; 0 and *sig_cap the signature slots it reserves, or FDGPU_ERR_INVAL
   with the error text set. */
int precompile_args(const fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_precompile_t const *tx,
                    uint64_t n, uint64_t *sig_cap) {
  if (!e || (!arena && arena_sz) || (!tx && n)) { set_err("null argument"); return FDGPU_ERR_INVAL; }
  if (n > e->cfg.max_txn || n > 0x7FFFFFFull) { set_err("batch exceeds engine limits"); return FDGPU_ERR_INVAL; }
  uint64_t cap = 0;
  for (uint64_t i = 0; i < n; i++) {
    if ((uint64_t)tx[i].off + tx[i].sz > arena_sz || tx[i].sz > FDT_TXN_MTU) {
      set_err("transaction %llu: out of the arena, or larger than %u bytes", (unsigned long long)i, (unsigned)FDT_TXN_MTU);
      return FDGPU_ERR_INVAL;
    }
    cap += tx[i].sig_cap;
  }
  if (cap > e->cfg.max_sig) {
    set_err("the batch reserves %llu signature slots, the engine holds %llu", (unsigned long long)cap,
            (unsigned long long)e->cfg.max_sig);
    return FDGPU_ERR_INVAL;
  }
  *sig_cap = cap;
  return FDGPU_OK;
}

/* the slot's precompile buffers, on its first such batch.  d_pc, whose presence says all are there, is allocated
   last: a failure part-way is retried by the next batch. */
bool slot_precompile_bufs(Slot &s, const fdgpu_cfg_t &c) {
  if (s.d_pc) return true;
  const uint64_t n = c.max_txn + 1;
  HIPCHK(s.h_pc.alloc(n * sizeof(fdgpu_precompile_t)), false);
  HIPCHK(s.d_pc_cnt.alloc(64), false);
  HIPCHK(s.d_pc_txn.alloc(n * FDT_TXN_MAX_SZ_BYTES), false);
  HIPCHK(s.d_pc_walk.alloc(n * sizeof(fdgpu_precompile_walk_t)), false);
  HIPCHK(s.d_pc_pos.alloc(c.max_sig * sizeof(uint32_t) + 16), false);
  HIPCHK(s.d_pc.alloc(n * sizeof(fdgpu_precompile_t)), false);
  return true;
}

}  // namespace fdgpu

namespace {

constexpr uint64_t INFO_SZ = sizeof(fdgpu_precompile_info_t);

/* a precompile batch resident on the device outside the ring (the diagnostics): synchronous upload */
struct DevPrecompiles {
  DevBuf<uint8_t> arena, res, txn_out;
  DevBuf<fdgpu_precompile_t> tx;
  DevBuf<fdgpu_sig_desc_t> sigs;
  DevBuf<fdgpu_precompile_walk_t> walk;
  DevBuf<uint32_t> cnt, pos;
  DevBuf<int8_t> sig_codes;
  uint64_t sig_cap = 0;
  int upload(fdgpu_engine_t *e, uint8_t const *a, uint64_t arena_sz, fdgpu_precompile_t const *t, uint64_t n) {
    if (!n) { set_err("empty batch"); return FDGPU_ERR_INVAL; }
    if (e && arena_sz > UINT32_MAX - 64ull * 1024) { set_err("arena too large"); return FDGPU_ERR_INVAL; }
    const int rc = precompile_args(e, a, arena_sz, t, n, &sig_cap);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
    HIPCHK(dev_arena(arena, a, arena_sz), FDGPU_ERR_DEVICE);
    if (res.alloc(item_results(n, INFO_SZ).bytes) || txn_out.alloc(n * FDT_TXN_MAX_SZ_BYTES) ||
        tx.alloc(n * sizeof(fdgpu_precompile_t)) || sigs.alloc(sig_cap * sizeof(fdgpu_sig_desc_t) + 16) ||
        walk.alloc(n * sizeof(fdgpu_precompile_walk_t)) || cnt.alloc(64) || pos.alloc(sig_cap * sizeof(uint32_t) + 16) ||
        sig_codes.alloc(sig_cap + 16)) {
      (void)hipGetLastError();
      set_err("alloc");
      return FDGPU_ERR_DEVICE;
    }
    HIPCHK(hipMemcpy(tx, t, n * sizeof(fdgpu_precompile_t), hipMemcpyHostToDevice), FDGPU_ERR_DEVICE);
    return FDGPU_OK;
  }
  int ingest(uint64_t n, hipStream_t st) {
    HIPCHK(hipMemsetAsync(cnt, 0, sizeof(uint32_t), st), FDGPU_ERR_DEVICE);
    HIPCHK(fdgpu_launch_precompile_ingest(arena, tx, (uint32_t)n, txn_out, sigs, pos, walk, cnt, st), FDGPU_ERR_DEVICE);
    return FDGPU_OK;
  }
};

}  // namespace

extern "C" {

uint32_t fdgpu_precompile_sig_bound(uint64_t sz) { return fdt_precompile_sig_bound(sz); }

int64_t fdgpu_submit_precompiles(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz,
                                 fdgpu_precompile_t const *txns, uint64_t n) {
  if (e && arena_sz > e->cfg.max_arena) { set_err("batch exceeds engine limits"); return FDGPU_ERR_INVAL; }
  uint64_t cap = 0;
  const int arc = precompile_args(e, arena, arena_sz, txns, n, &cap);
  if (arc) return arc;
  std::lock_guard<std::mutex> lk(e->ring_mu);
  Slot *s = nullptr;
  if (const int rc = take_slot(e, &s)) return rc;
  if (!n) return slot_publish(e, s, Batch::Precompile, 0, 0, 0);
  if (!slot_precompile_bufs(*s, e->cfg) || !slot_res_bufs(*s, e->cfg) || (cap && !slot_ws(*s, cap))) return FDGPU_ERR_DEVICE;
  if (const int rc = slot_upload(e, s, arena, arena_sz)) return rc;
  const ItemResults res = item_results(n, INFO_SZ);
  memcpy(s->h_pc, txns, n * sizeof(fdgpu_precompile_t));
  HIPCHK(hipMemcpyAsync(s->d_pc, s->h_pc, n * sizeof(fdgpu_precompile_t), hipMemcpyHostToDevice, s->stream), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemsetAsync(s->d_pc_cnt, 0, sizeof(uint32_t), s->stream), FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_precompile_ingest(s->d_arena, s->d_pc, (uint32_t)n, s->d_pc_txn, s->d_sigs, s->d_pc_pos, s->d_pc_walk,
                                        s->d_pc_cnt, s->stream),
         FDGPU_ERR_DEVICE);
  /* the reserved slots bound the signature count (a transaction never takes more than its sig_cap); the count itself
     stays on the device.  A batch that reserves none has nothing to verify. */
  if (cap)
    HIPCHK(fdgpu_launch_verify_sigs(s->d_arena, s->d_sigs, (uint32_t)cap, nullptr, e->d_btab, s->d_ws, s->d_sig_codes,
                                    ring_kflags(e, s, cap), s->stream, s->d_pc_cnt, e->resident_blocks, e->kc_seed),
           FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_precompile_finish(s->d_pc_walk, (uint32_t)n, s->d_sig_codes, s->d_pc_pos, (int8_t *)s->d_res.p,
                                        s->d_res + res.items, s->stream),
         FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpyAsync(s->h_res, s->d_res, res.bytes, hipMemcpyDeviceToHost, s->stream), FDGPU_ERR_DEVICE);
  return slot_publish(e, s, Batch::Precompile, n, 0, 0);
}

int fdgpu_poll_precompiles(fdgpu_engine_t *e, int64_t ticket, int8_t *codes, fdgpu_precompile_info_t *info, int blocking) {
  return poll_slot(e, ticket, codes, blocking, false, nullptr, nullptr, nullptr, (uint8_t *)info);
}

int fdgpu_debug_precompile_walk(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_precompile_t const *txns,
                                uint64_t n, fdgpu_precompile_walk_t *walk, uint32_t *descs, uint32_t *pos,
                                uint64_t desc_cap, uint64_t *desc_cnt) {
  if (!walk || !desc_cnt) { set_err("null argument"); return FDGPU_ERR_INVAL; }
  DevPrecompiles b;
  int rc = b.upload(e, arena, arena_sz, txns, n);
  if (rc) return rc;
  if ((descs || pos) && desc_cap < b.sig_cap) { set_err("desc_cap below the reserved signature slots"); return FDGPU_ERR_INVAL; }
  rc = b.ingest(n, e->compute);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
  uint32_t cnt = 0;
  HIPCHK(hipMemcpy(&cnt, b.cnt, sizeof cnt, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  if (cnt > b.sig_cap) { set_err("the ingest took %u slots of %llu", cnt, (unsigned long long)b.sig_cap); return FDGPU_ERR_DEVICE; }
  HIPCHK(hipMemcpy(walk, b.walk, n * sizeof(fdgpu_precompile_walk_t), hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  if (descs && cnt) HIPCHK(hipMemcpy(descs, b.sigs, cnt * sizeof(fdgpu_sig_desc_t), hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  if (pos && cnt) HIPCHK(hipMemcpy(pos, b.pos, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  *desc_cnt = cnt;
  return FDGPU_OK;
}

int fdgpu_debug_precompile_time(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_precompile_t const *txns,
                                uint64_t n, int iters, double *ingest_ms, double *verify_ms) {
  if (iters < 1 || !ingest_ms || !verify_ms) { set_err("bad argument"); return FDGPU_ERR_INVAL; }
  DevPrecompiles b;
  int rc = b.upload(e, arena, arena_sz, txns, n);
  if (rc) return rc;
  if (!b.sig_cap) { set_err("the batch reserves no signature slots"); return FDGPU_ERR_INVAL; }
  if (b.sig_cap > e->ws_sig) {
    HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
    rc = ensure_ws(e, b.sig_cap);
    if (rc) return rc;
  }
  hipStream_t st = e->compute;
  /* the warm-up also leaves the descriptors and the count the timed verifies read */
  auto ingest = [&] { return !b.ingest(n, st); };
  auto verify = [&] {
    return fdgpu_launch_verify_sigs(b.arena, b.sigs, (uint32_t)b.sig_cap, nullptr, e->d_btab, e->d_ws, b.sig_codes,
                                    kflags(e), st, b.cnt, e->resident_blocks, e->kc_seed) == hipSuccess;
  };
  return time_two_stages(st, iters, "precompile", [&] { return ingest() && verify(); }, ingest, verify, ingest_ms,
                         verify_ms);
}

}  // extern "C"
