/* fdt_callers.cpp -- the other callers of the verify API, batched over a
   verifier:

     replay   fd_executor_txn_verify (src/flamenco/runtime/fd_executor.c:
              1157-1185) runs fd_ed25519_verify_batch_single_msg on each
              parsed transaction of a block, one at a time;
              fdgpu_replay_verify takes a whole block's raw transactions,
              parses them (fdt_txn_parse) and verifies them in batches;
     shreds   fd_fec_resolver.c:438 checks each new FEC set's merkle root
              with fd_ed25519_verify(root, 32, sig, leader_pubkey);
              fdgpu_fec_roots_verify verifies many roots in one batch
              (32-byte messages, single signatures);
              fdgpu_shreds_verify starts from the raw shreds: the checks
              before the signature and the SHA-256 Merkle root on the host
              (fdt_shred.h), then the same batched verify;
     poh      fd_runtime_block_verify_tpool (src/flamenco/runtime/
              fd_runtime.c:2274-2371) hashes every microblock's chain, builds
              the Merkle root of its signatures and mixes it in;
              fdgpu_block_poh_verify takes the entries of many blocks and
              their raw transactions and runs them as PoH batches on the
              engine (fd_poh_gpu.h), fdgpu_poh_verify_host on the host.

   Both cut the work into batches within the verifier's limits, keep up to
   two batches in flight (the next one is staged while the GPU runs the
   previous) and return one fd_ed25519 code per item. */
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "../../../include/fd_verify_tile.h"
#include "../fdt_poh.h"
#include "../fdt_shred.h"

namespace {

struct Chunk {
  std::vector<uint8_t> arena;
  std::vector<fdgpu_txn_t> txns;
  std::vector<uint64_t> items;     /* caller's index of each txn */
  int64_t ticket = -1;
};

/* Submit / poll with at most two chunks in flight; codes written per item. */
struct Pipe {
  Pipe(fdgpu_verifier_t v_, int8_t *codes_) : v(v_), codes(codes_) {}
  fdgpu_verifier_t v;
  int8_t *codes;
  Chunk slot[2];
  int head = 0, cnt = 0;
  std::vector<int8_t> buf;

  int drain_one() {
    Chunk &c = slot[head];
    buf.resize(std::max<size_t>(c.txns.size(), 1));
    const int r = v.poll(v.ctx, c.ticket, buf.data(), 1);
    if (r != FDGPU_OK) return r < 0 ? r : FDGPU_ERR_DEVICE;
    for (size_t i = 0; i < c.items.size(); i++) codes[c.items[i]] = buf[i];
    head ^= 1;
    cnt--;
    return 0;
  }

  /* the chunk to fill next (drains the oldest when both are busy) */
  int next(Chunk **out) {
    if (cnt == 2) {
      const int r = drain_one();
      if (r) return r;
    }
    Chunk &c = slot[(head + cnt) & 1];
    c.arena.clear(); c.txns.clear(); c.items.clear();
    *out = &c;
    return 0;
  }

  int submit(Chunk &c) {
    if (c.txns.empty()) return 0;
    int64_t tk;
    while ((tk = v.submit(v.ctx, c.arena.data(), c.arena.size(), c.txns.data(), c.txns.size())) == FDGPU_ERR_FULL) {
      if (!cnt) return FDGPU_ERR_FULL;
      const int r = drain_one();
      if (r) return r;
    }
    if (tk < 0) return (int)tk;
    c.ticket = tk;
    cnt++;
    return 0;
  }

  int finish() {
    while (cnt) {
      const int r = drain_one();
      if (r) return r;
    }
    return 0;
  }
};

}  // namespace

extern "C" {

int fdgpu_replay_verify(fdgpu_verifier_t v, const uint8_t *payloads, const uint64_t *off, const uint32_t *sz,
                        uint64_t n, uint64_t batch_txn_max, uint64_t batch_bytes_max, int8_t *codes) {
  if (!v.submit || !v.poll || !codes || (n && (!payloads || !off || !sz)) || !batch_txn_max ||
      batch_bytes_max < FDT_TXN_MTU)
    return FDGPU_ERR_INVAL;
  Pipe p(v, codes);
  alignas(8) uint8_t txn_buf[FDT_TXN_MAX_SZ];
  Chunk *c = nullptr;
  int r = p.next(&c);
  for (uint64_t i = 0; i < n && !r; i++) {
    const uint8_t *raw = payloads + off[i];
    const uint64_t psz = std::min<uint64_t>(sz[i], FDT_TXN_MTU);
    if (!fdt_txn_parse(raw, psz, txn_buf, nullptr)) { codes[i] = FDGPU_REPLAY_PARSE_FAIL; continue; }
    const fdt_txn_t *t = (const fdt_txn_t *)txn_buf;
    if (c->txns.size() == batch_txn_max || c->arena.size() + psz > batch_bytes_max) {
      r = p.submit(*c);
      if (!r) r = p.next(&c);
      if (r) break;
    }
    const uint32_t base = (uint32_t)c->arena.size();
    c->arena.insert(c->arena.end(), raw, raw + psz);
    /* the descriptor fields fd_executor_txn_verify reads (fd_executor.c:1167-1175) */
    fdgpu_txn_t d;
    d.sig_off = base + t->signature_off;
    d.pub_off = base + t->acct_addr_off;
    d.msg_off = base + t->message_off;
    d.msg_sz = (uint32_t)(psz - t->message_off);
    d.sig_cnt = t->signature_cnt;
    c->txns.push_back(d);
    c->items.push_back(i);
  }
  if (!r) r = p.submit(*c);
  if (!r) r = p.finish();
  return r;
}

int fdgpu_fec_roots_verify(fdgpu_verifier_t v, const uint8_t *roots, const uint8_t *sigs, const uint8_t *pubkeys,
                           int shared_pubkey, uint64_t n, uint64_t batch_max, int8_t *codes) {
  if (!v.submit || !v.poll || !codes || (n && (!roots || !sigs || !pubkeys)) || !batch_max)
    return FDGPU_ERR_INVAL;
  Pipe p(v, codes);
  Chunk *c = nullptr;
  int r = p.next(&c);
  for (uint64_t i = 0; i < n && !r; i++) {
    if (c->txns.size() == batch_max) {
      r = p.submit(*c);
      if (!r) r = p.next(&c);
      if (r) break;
    }
    /* item = sig[64] | pub[32] | root[32]: fd_ed25519_verify(root, 32, sig, pub) */
    const uint32_t base = (uint32_t)c->arena.size();
    c->arena.insert(c->arena.end(), sigs + 64 * i, sigs + 64 * i + 64);
    const uint8_t *pk = pubkeys + (shared_pubkey ? 0 : 32 * i);
    c->arena.insert(c->arena.end(), pk, pk + 32);
    c->arena.insert(c->arena.end(), roots + 32 * i, roots + 32 * i + 32);
    fdgpu_txn_t d;
    d.sig_off = base;
    d.pub_off = base + 64;
    d.msg_off = base + 96;
    d.msg_sz = 32;
    d.sig_cnt = 1;
    c->txns.push_back(d);
    c->items.push_back(i);
  }
  if (!r) r = p.submit(*c);
  if (!r) r = p.finish();
  return r;
}

int fdt_shred_check(const uint8_t *buf, uint64_t sz, uint16_t expected_version, fdt_shred_chk_t *out) {
  fdt_shred_chk_t tmp;
  const int ok = fdt_shred_check_core(buf, sz, expected_version, &tmp);
  if (ok && out) *out = tmp;
  return ok;
}

void fdt_shred_root(const uint8_t *buf, const fdt_shred_chk_t *chk, uint8_t *root) { fdt_shred_root_core(buf, chk, root); }

void fdt_sha256(const uint8_t *data, uint64_t sz, uint8_t *out) {
  fdt_sha256_t s;
  fdt_sha256_init(&s);
  fdt_sha256_append(&s, data, sz);
  fdt_sha256_fini(&s, out);
}

int fdgpu_shreds_verify(fdgpu_verifier_t v, const uint8_t *arena, uint64_t arena_sz, const fdgpu_shred_t *shreds,
                        uint64_t n, uint16_t expected_version, uint64_t batch_max, int8_t *codes, uint8_t *roots) {
  if (!v.submit || !v.poll || !codes || (n && (!arena || !shreds)) || !batch_max) return FDGPU_ERR_INVAL;
  for (uint64_t i = 0; i < n; i++)
    if ((uint64_t)shreds[i].off + shreds[i].sz > arena_sz || (uint64_t)shreds[i].pub_off + 32 > arena_sz)
      return FDGPU_ERR_INVAL;
  /* the roots first, shreds dealt to the threads in runs of 256 (a shred's hash is ~40 SHA-256 blocks) */
  std::vector<uint8_t> own;
  if (!roots) { own.resize(32 * std::max<uint64_t>(n, 1)); roots = own.data(); }
  std::vector<uint8_t> ok(std::max<uint64_t>(n, 1));
  std::atomic<uint64_t> next{0};
  auto work = [&] {
    for (uint64_t b; (b = next.fetch_add(256)) < n;)
      for (uint64_t i = b; i < std::min(n, b + 256); i++) {
        fdt_shred_chk_t chk;
        ok[i] = (uint8_t)fdt_shred_check_core(arena + shreds[i].off, shreds[i].sz, expected_version, &chk);
        if (ok[i]) fdt_shred_root_core(arena + shreds[i].off, &chk, roots + 32 * i);
        else memset(roots + 32 * i, 0, 32);
      }
  };
  const unsigned hw = std::thread::hardware_concurrency();
  const uint64_t nt = std::min<uint64_t>({16, hw ? hw : 1, (n + 1023) / 1024});
  std::vector<std::thread> th;
  for (uint64_t t = 1; t < nt; t++) th.emplace_back(work);
  work();
  for (auto &t : th) t.join();
  Pipe p(v, codes);
  Chunk *c = nullptr;
  int r = p.next(&c);
  for (uint64_t i = 0; i < n && !r; i++) {
    if (!ok[i]) { codes[i] = FDGPU_CODE_SHRED_REJECT; continue; }
    if (c->txns.size() == batch_max) {
      r = p.submit(*c);
      if (!r) r = p.next(&c);
      if (r) break;
    }
    /* item = sig[64] | pub[32] | root[32], as fdgpu_fec_roots_verify */
    const uint32_t base = (uint32_t)c->arena.size();
    const uint8_t *sh = arena + shreds[i].off, *pk = arena + shreds[i].pub_off;
    c->arena.insert(c->arena.end(), sh, sh + 64);
    c->arena.insert(c->arena.end(), pk, pk + 32);
    c->arena.insert(c->arena.end(), roots + 32 * i, roots + 32 * i + 32);
    fdgpu_txn_t d;
    d.sig_off = base;
    d.pub_off = base + 64;
    d.msg_off = base + 96;
    d.msg_sz = 32;
    d.sig_cnt = 1;
    c->txns.push_back(d);
    c->items.push_back(i);
  }
  if (!r) r = p.submit(*c);
  if (!r) r = p.finish();
  return r;
}

int fdgpu_poh_verify_host(const uint8_t *arena, uint64_t arena_sz, const fdgpu_poh_entry_t *entries, uint64_t n,
                          const uint32_t *sig_offs, uint64_t sig_total, uint64_t hash_cnt_cap, int8_t *codes,
                          uint8_t *hashes) {
  if (!codes || (!arena && arena_sz) || (!entries && n) || (!sig_offs && sig_total)) return FDGPU_ERR_INVAL;
  uint64_t bad;
  if (fdt_poh_args(arena_sz, entries, n, sig_offs, sig_total, hash_cnt_cap, &bad)) return FDGPU_ERR_INVAL;
  /* entries dealt to the threads one at a time: their lengths differ by orders of magnitude */
  std::atomic<uint64_t> next{0};
  auto work = [&] {
    std::vector<uint8_t> nodes;
    uint8_t out[32];
    for (uint64_t i; (i = next.fetch_add(1)) < n;) {
      nodes.resize(32 * std::max<uint64_t>(entries[i].sig_cnt, 1));
      codes[i] = (int8_t)fdt_poh_entry(arena, entries + i, sig_offs, hash_cnt_cap, nodes.data(), out);
      if (hashes) memcpy(hashes + 32 * i, out, 32);
    }
  };
  const unsigned hw = std::thread::hardware_concurrency();
  const uint64_t nt = std::min<uint64_t>({16, hw ? hw : 1, n});
  std::vector<std::thread> th;
  for (uint64_t t = 1; t < nt; t++) th.emplace_back(work);
  work();
  for (auto &t : th) t.join();
  return FDGPU_OK;
}

int fdgpu_block_poh_verify(fdgpu_engine_t *e, const uint8_t in_hash[32], const uint64_t *hash_cnt, const uint8_t *entry_hash,
                           const uint32_t *txn_cnt, uint64_t m, const uint8_t *payloads, const uint64_t *off,
                           const uint32_t *sz, uint64_t n_txn, uint64_t hash_cnt_cap, uint64_t batch_entry_max,
                           int8_t *codes) {
  if (!codes || !batch_entry_max || (m && (!in_hash || !hash_cnt || !entry_hash || !txn_cnt)) ||
      (n_txn && (!payloads || !off || !sz)) || hash_cnt_cap < 1 || hash_cnt_cap > FDGPU_POH_HASH_CNT_MAX)
    return FDGPU_ERR_INVAL;
  uint64_t tot = 0;
  for (uint64_t i = 0; i < m; i++) tot += txn_cnt[i];
  if (tot != n_txn) return FDGPU_ERR_INVAL;
  uint64_t entry_max = batch_entry_max, sig_max = UINT32_MAX, arena_max = UINT32_MAX - 64ull * 1024;
  if (e) {
    uint64_t em = 0;
    if (fdgpu_poh_limits(e, &em, &sig_max, &arena_max)) return FDGPU_ERR_INVAL;
    entry_max = std::min(entry_max, em);
  }
  /* a batch: per entry its start hash, its claimed hash and its signatures, copied into an arena of the batch's own */
  struct PohChunk {
    std::vector<uint8_t> arena;
    std::vector<fdgpu_poh_entry_t> en;
    std::vector<uint32_t> so;
    std::vector<uint64_t> items;   /* caller's index of each entry */
    int64_t ticket = -1;
  } slot[2];
  int head = 0, cnt = 0;
  std::vector<int8_t> buf;
  auto drain_one = [&]() -> int {
    PohChunk &c = slot[head];
    buf.resize(std::max<size_t>(c.en.size(), 1));
    const int r = fdgpu_poll_poh(e, c.ticket, buf.data(), nullptr, 1);
    if (r != FDGPU_OK) return r < 0 ? r : FDGPU_ERR_DEVICE;
    for (size_t i = 0; i < c.items.size(); i++) codes[c.items[i]] = buf[i];
    head ^= 1;
    cnt--;
    return 0;
  };
  auto next = [&](PohChunk **out) -> int {     /* the chunk to fill next (drains the oldest when both are busy) */
    if (cnt == 2) {
      const int r = drain_one();
      if (r) return r;
    }
    PohChunk &c = slot[(head + cnt) & 1];
    c.arena.clear(); c.en.clear(); c.so.clear(); c.items.clear();
    *out = &c;
    return 0;
  };
  auto submit = [&](PohChunk &c) -> int {
    if (c.en.empty()) return 0;
    if (!e) {
      buf.resize(c.en.size());
      const int r = fdgpu_poh_verify_host(c.arena.data(), c.arena.size(), c.en.data(), c.en.size(), c.so.data(),
                                          c.so.size(), hash_cnt_cap, buf.data(), nullptr);
      if (r) return r;
      for (size_t i = 0; i < c.items.size(); i++) codes[c.items[i]] = buf[i];
      return 0;
    }
    int64_t tk;
    while ((tk = fdgpu_submit_poh(e, c.arena.data(), c.arena.size(), c.en.data(), c.en.size(), c.so.data(), c.so.size(),
                                  hash_cnt_cap)) == FDGPU_ERR_FULL) {
      if (!cnt) return FDGPU_ERR_FULL;
      const int r = drain_one();
      if (r) return r;
    }
    if (tk < 0) return (int)tk;
    c.ticket = tk;
    cnt++;
    return 0;
  };
  alignas(8) uint8_t txn_buf[FDT_TXN_MAX_SZ];
  std::vector<uint64_t> sig_at;                /* an entry's signatures: where they lie in payloads */
  PohChunk *c = nullptr;
  int r = next(&c);
  uint64_t t = 0;
  for (uint64_t i = 0; i < m && !r; t += txn_cnt[i], i++) {
    bool parsed = true;
    sig_at.clear();
    for (uint64_t j = t; j < t + txn_cnt[i] && parsed; j++) {
      const uint8_t *raw = payloads + off[j];
      const uint64_t psz = std::min<uint64_t>(sz[j], FDT_TXN_MTU);
      if (!fdt_txn_parse(raw, psz, txn_buf, nullptr)) { parsed = false; break; }
      const fdt_txn_t *tx = (const fdt_txn_t *)txn_buf;
      for (uint64_t k = 0; k < tx->signature_cnt; k++) sig_at.push_back(off[j] + tx->signature_off + 64 * k);
    }
    if (!parsed) { codes[i] = FDGPU_REPLAY_PARSE_FAIL; continue; }
    const uint64_t need = 64 + 64 * sig_at.size();
    if (sig_at.size() > sig_max || need > arena_max) { r = FDGPU_ERR_INVAL; break; }   /* one entry no batch can hold */
    if (c->en.size() == entry_max || c->so.size() + sig_at.size() > sig_max || c->arena.size() + need > arena_max) {
      r = submit(*c);
      if (!r) r = next(&c);
      if (r) break;
    }
    /* item = start hash[32] | claimed hash[32] | its signatures[64 each] */
    const uint32_t base = (uint32_t)c->arena.size();
    const uint8_t *prev = i ? entry_hash + 32 * (i - 1) : in_hash;
    c->arena.insert(c->arena.end(), prev, prev + 32);
    c->arena.insert(c->arena.end(), entry_hash + 32 * i, entry_hash + 32 * i + 32);
    fdgpu_poh_entry_t d;
    d.hash_cnt = hash_cnt[i];
    d.prev_off = base;
    d.hash_off = base + 32;
    d.sig_first = (uint32_t)c->so.size();
    d.sig_cnt = (uint32_t)sig_at.size();
    d.mix_off = FDGPU_POH_NO_MIX;
    d._pad = 0;
    for (uint64_t at : sig_at) {
      c->so.push_back((uint32_t)c->arena.size());
      c->arena.insert(c->arena.end(), payloads + at, payloads + at + 64);
    }
    c->en.push_back(d);
    c->items.push_back(i);
  }
  if (!r) r = submit(*c);
  while (cnt) {                                /* on an error too: no batch is left in the ring */
    const int d = drain_one();
    if (d) return r ? r : d;
  }
  return r;
}

}  // extern "C"
