/* fdgpu_secp256k1s.cpp -- a block's secp256k1 precompile instructions through the engine (include/fd_secp256k1_gpu.h):
   the ring batch (fdgpu_submit_secp256k1 / fdgpu_poll_secp256k1) and the diagnostics.  A batch is its arena uploaded
   as any frag batch's, then on the slot's stream ingest (parse, the walk over the record tables, one descriptor per
   record that resolves) -> recover (one code per record) -> finish (codes and infos side by side) and one read-back.
   It uses the slot buffers of fdgpu_precompiles.cpp's batches: a slot carries one batch at a time. */
#include "fdgpu_engine.h"
#include "fdgpu_secp256k1.h"
#include "fdt_secp256k1.h"

using namespace fdgpu;

static_assert(FDGPU_SECP256K1_FAIL_ON_BAD_COUNT == FDT_SECP256K1_FAIL_ON_BAD_COUNT, "the walk reads the public flag");

namespace {

constexpr uint64_t INFO_SZ = sizeof(fdgpu_precompile_info_t);

bool flags_ok(uint32_t flags) {
  if (flags & ~FDGPU_SECP256K1_FAIL_ON_BAD_COUNT) { set_err("unknown flag"); return false; }
  return true;
}

/* a batch resident on the device outside the ring (the diagnostics): synchronous upload */
struct DevSecp256k1 {
  DevBuf<uint8_t> arena, txn_out;
  DevBuf<fdgpu_precompile_t> tx;
  DevBuf<fdgpu_sig_desc_t> descs;
  DevBuf<fdgpu_precompile_walk_t> walk;
  DevBuf<uint32_t> cnt, pos;
  DevBuf<int8_t> rec_codes;
  uint64_t cap = 0;
  uint32_t flags = 0;
  int upload(fdgpu_engine_t *e, uint8_t const *a, uint64_t arena_sz, fdgpu_precompile_t const *t, uint64_t n, uint32_t fl) {
    if (!n) { set_err("empty batch"); return FDGPU_ERR_INVAL; }
    if (!flags_ok(fl)) return FDGPU_ERR_INVAL;
    if (e && arena_sz > UINT32_MAX - 64ull * 1024) { set_err("arena too large"); return FDGPU_ERR_INVAL; }
    const int rc = precompile_args(e, a, arena_sz, t, n, &cap);
    if (rc) return rc;
    flags = fl;
    HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
    HIPCHK(dev_arena(arena, a, arena_sz), FDGPU_ERR_DEVICE);
    if (txn_out.alloc(n * FDT_TXN_MAX_SZ_BYTES) || tx.alloc(n * sizeof(fdgpu_precompile_t)) ||
        descs.alloc(cap * sizeof(fdgpu_sig_desc_t) + 16) || walk.alloc(n * sizeof(fdgpu_precompile_walk_t)) ||
        cnt.alloc(64) || pos.alloc(cap * sizeof(uint32_t) + 16) || rec_codes.alloc(cap + 16)) {
      (void)hipGetLastError();
      set_err("alloc");
      return FDGPU_ERR_DEVICE;
    }
    HIPCHK(hipMemcpy(tx, t, n * sizeof(fdgpu_precompile_t), hipMemcpyHostToDevice), FDGPU_ERR_DEVICE);
    return FDGPU_OK;
  }
  int ingest(uint64_t n, hipStream_t st) {
    HIPCHK(hipMemsetAsync(cnt, 0, sizeof(uint32_t), st), FDGPU_ERR_DEVICE);
    HIPCHK(fdgpu_launch_secp256k1_ingest(arena, tx, (uint32_t)n, flags, txn_out, descs, pos, walk, cnt, st), FDGPU_ERR_DEVICE);
    return FDGPU_OK;
  }
};

}  // namespace

extern "C" {

uint32_t fdgpu_secp256k1_sig_bound(uint64_t sz) { return fdt_secp256k1_sig_bound(sz); }

int64_t fdgpu_submit_secp256k1(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_precompile_t const *txns,
                               uint64_t n, uint32_t flags) {
  if (!flags_ok(flags)) return FDGPU_ERR_INVAL;
  if (e && arena_sz > e->cfg.max_arena) { set_err("batch exceeds engine limits"); return FDGPU_ERR_INVAL; }
  uint64_t cap = 0;
  const int arc = precompile_args(e, arena, arena_sz, txns, n, &cap);
  if (arc) return arc;
  std::lock_guard<std::mutex> lk(e->ring_mu);
  Slot *s = nullptr;
  if (const int rc = take_slot(e, &s)) return rc;
  if (!n) return slot_publish(e, s, Batch::Secp256k1, 0, 0, 0);
  if (!slot_precompile_bufs(*s, e->cfg) || !slot_res_bufs(*s, e->cfg)) return FDGPU_ERR_DEVICE;
  if (const int rc = slot_upload(e, s, arena, arena_sz)) return rc;
  const ItemResults res = item_results(n, INFO_SZ);
  memcpy(s->h_pc, txns, n * sizeof(fdgpu_precompile_t));
  HIPCHK(hipMemcpyAsync(s->d_pc, s->h_pc, n * sizeof(fdgpu_precompile_t), hipMemcpyHostToDevice, s->stream), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemsetAsync(s->d_pc_cnt, 0, sizeof(uint32_t), s->stream), FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_secp256k1_ingest(s->d_arena, s->d_pc, (uint32_t)n, flags, s->d_pc_txn, s->d_sigs, s->d_pc_pos,
                                       s->d_pc_walk, s->d_pc_cnt, s->stream),
         FDGPU_ERR_DEVICE);
  /* the reserved slots bound the record count (a transaction never takes more than its sig_cap); the count itself stays
     on the device.  A batch that reserves none has nothing to recover. */
  HIPCHK(fdgpu_launch_secp256k1_recover(s->d_arena, s->d_sigs, (uint32_t)cap, s->d_pc_cnt, s->d_sig_codes, s->stream),
         FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_secp256k1_finish(s->d_pc_walk, (uint32_t)n, s->d_sig_codes, s->d_pc_pos, (int8_t *)s->d_res.p,
                                       s->d_res + res.items, s->stream),
         FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpyAsync(s->h_res, s->d_res, res.bytes, hipMemcpyDeviceToHost, s->stream), FDGPU_ERR_DEVICE);
  return slot_publish(e, s, Batch::Secp256k1, n, 0, 0);
}

int fdgpu_poll_secp256k1(fdgpu_engine_t *e, int64_t ticket, int8_t *codes, fdgpu_precompile_info_t *info, int blocking) {
  return poll_slot(e, ticket, codes, blocking, false, nullptr, nullptr, nullptr, (uint8_t *)info);
}

int fdgpu_debug_secp256k1_walk(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_precompile_t const *txns,
                               uint64_t n, uint32_t flags, fdgpu_precompile_walk_t *walk, uint32_t *descs, uint32_t *pos,
                               uint64_t desc_cap, uint64_t *desc_cnt) {
  if (!walk || !desc_cnt) { set_err("null argument"); return FDGPU_ERR_INVAL; }
  DevSecp256k1 b;
  int rc = b.upload(e, arena, arena_sz, txns, n, flags);
  if (rc) return rc;
  if ((descs || pos) && desc_cap < b.cap) { set_err("desc_cap below the reserved record slots"); return FDGPU_ERR_INVAL; }
  rc = b.ingest(n, e->compute);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
  uint32_t cnt = 0;
  HIPCHK(hipMemcpy(&cnt, b.cnt, sizeof cnt, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  if (cnt > b.cap) { set_err("the ingest took %u slots of %llu", cnt, (unsigned long long)b.cap); return FDGPU_ERR_DEVICE; }
  HIPCHK(hipMemcpy(walk, b.walk, n * sizeof(fdgpu_precompile_walk_t), hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  if (descs && cnt) HIPCHK(hipMemcpy(descs, b.descs, cnt * sizeof(fdgpu_sig_desc_t), hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  if (pos && cnt) HIPCHK(hipMemcpy(pos, b.pos, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  *desc_cnt = cnt;
  return FDGPU_OK;
}

int fdgpu_debug_keccak256(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, uint32_t const *off_sz, uint64_t n,
                          uint8_t *digests) {
  if (!e || !n || !off_sz || !digests || (!arena && arena_sz)) { set_err("bad argument"); return FDGPU_ERR_INVAL; }
  if (n > 0x7FFFFFFull || arena_sz > UINT32_MAX - 64ull * 1024) { set_err("batch too large"); return FDGPU_ERR_INVAL; }
  for (uint64_t i = 0; i < n; i++)
    if ((uint64_t)off_sz[2 * i] + off_sz[2 * i + 1] > arena_sz || off_sz[2 * i + 1] > FDT_TXN_MTU) {
      set_err("message %llu: out of the arena, or longer than %u bytes", (unsigned long long)i, (unsigned)FDT_TXN_MTU);
      return FDGPU_ERR_INVAL;
    }
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  DevBuf<uint8_t> d_arena;
  DevBuf<uint32_t> d_os, d_out;
  HIPCHK(dev_arena(d_arena, arena, arena_sz), FDGPU_ERR_DEVICE);
  HIPCHK(d_os.alloc(n * 8), FDGPU_ERR_DEVICE);
  HIPCHK(d_out.alloc(n * 32), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(d_os, off_sz, n * 8, hipMemcpyHostToDevice), FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_test_keccak256(d_arena, d_os, (uint32_t)n, d_out, e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(digests, d_out, n * 32, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

int fdgpu_debug_secp256k1_recover(fdgpu_engine_t *e, uint8_t const *in, uint64_t n, int8_t *codes, uint8_t *keys) {
  if (!e || !n || !in || !codes || !keys) { set_err("bad argument"); return FDGPU_ERR_INVAL; }
  if (n > 0xFFFFFFull) { set_err("batch too large"); return FDGPU_ERR_INVAL; }
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  DevBuf<uint8_t> d_in;
  DevBuf<int8_t> d_codes;
  DevBuf<uint32_t> d_keys;
  HIPCHK(dev_arena(d_in, in, n * 97), FDGPU_ERR_DEVICE);      /* with the slack the reader's windows may touch */
  HIPCHK(d_codes.alloc(n), FDGPU_ERR_DEVICE);
  HIPCHK(d_keys.alloc(n * 64), FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_test_secp256k1_recover(d_in, (uint32_t)n, d_codes, d_keys, e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(codes, d_codes, n, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(keys, d_keys, n * 64, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

int fdgpu_debug_secp256k1_ops(fdgpu_engine_t *e, uint32_t const *in, uint64_t n, uint32_t *out) {
  if (!e || !n || !in || !out) { set_err("bad argument"); return FDGPU_ERR_INVAL; }
  if (n > 0xFFFFFFull) { set_err("batch too large"); return FDGPU_ERR_INVAL; }
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  DevBuf<uint32_t> d_in, d_out;
  HIPCHK(d_in.alloc(n * FDGPU_SECP256K1_OPS_IN * 4), FDGPU_ERR_DEVICE);
  HIPCHK(d_out.alloc(n * FDGPU_SECP256K1_OPS_OUT * 4), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(d_in, in, n * FDGPU_SECP256K1_OPS_IN * 4, hipMemcpyHostToDevice), FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_test_secp256k1_ops(d_in, d_out, (uint32_t)n, e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(out, d_out, n * FDGPU_SECP256K1_OPS_OUT * 4, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

int fdgpu_debug_secp256k1_time(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_precompile_t const *txns,
                               uint64_t n, uint32_t flags, int iters, double *ingest_ms, double *recover_ms) {
  if (iters < 1 || !ingest_ms || !recover_ms) { set_err("bad argument"); return FDGPU_ERR_INVAL; }
  DevSecp256k1 b;
  const int rc = b.upload(e, arena, arena_sz, txns, n, flags);
  if (rc) return rc;
  if (!b.cap) { set_err("the batch reserves no record slots"); return FDGPU_ERR_INVAL; }
  hipStream_t st = e->compute;
  /* the warm-up also leaves the descriptors and the count the timed recovers read */
  auto ingest = [&] { return !b.ingest(n, st); };
  auto recover = [&] {
    return fdgpu_launch_secp256k1_recover(b.arena, b.descs, (uint32_t)b.cap, b.cnt, b.rec_codes, st) == hipSuccess;
  };
  return time_two_stages(st, iters, "secp256k1", [&] { return ingest() && recover(); }, ingest, recover, ingest_ms,
                         recover_ms);
}

}  // extern "C"
