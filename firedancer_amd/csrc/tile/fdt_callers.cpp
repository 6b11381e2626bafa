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
              fdgpu_shred_sets_verify takes every shred of the sets
              (fd_fec_resolver.c:466-484 checks no signature after a set's
              first): one verify per distinct (signature, root, leader),
              shreds with a known root compared with it (fd_shred_sets_gpu.h);
     poh      fd_runtime_block_verify_tpool (src/flamenco/runtime/
              fd_runtime.c:2274-2371) hashes every microblock's chain, builds
              the Merkle root of its signatures and mixes it in;
              fdgpu_block_poh_verify takes the entries of many blocks and
              their raw transactions and runs them as PoH batches on the
              engine (fd_poh_gpu.h), fdgpu_poh_verify_host on the host;
     precompiles  fd_executor_verify_precompiles (src/flamenco/runtime/
              fd_executor.c:252-270) walks each transaction's Ed25519
              precompile instructions and runs fd_ed25519_verify on every
              record of their tables; fdgpu_precompiles_verify walks on the
              host (fdt_precompile.h) and verifies the records in batches,
              fdgpu_block_precompile_verify sends a block's transactions
              that carry such instructions through the engine
              (fd_precompile_gpu.h).

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
#include "../fdt_precompile.h"
#include "../fdt_secp256k1.h"
#include "../fdt_shred.h"
#include "../fdt_shred_sets.h"

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

int fdgpu_shred_sets_verify(fdgpu_verifier_t v, const uint8_t *arena, uint64_t arena_sz, const fdgpu_set_shred_t *shreds,
                            uint64_t n, uint16_t expected_version, uint64_t batch_max, int8_t *codes, uint8_t *roots,
                            uint32_t *rep, uint64_t *lanes) {
  if (!v.submit || !v.poll || !codes || (n && (!arena || !shreds)) || !batch_max) return FDGPU_ERR_INVAL;
  if (!fdt_shred_sets_args(arena_sz, shreds, n)) return FDGPU_ERR_INVAL;
  /* the roots first, as fdgpu_shreds_verify: shreds dealt to the threads in runs of 256 */
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
  /* the states, and one representative per distinct key: the first shred that carries it */
  std::vector<uint32_t> own_rep;
  if (!rep) { own_rep.resize(std::max<uint64_t>(n, 1)); rep = own_rep.data(); }
  std::vector<uint32_t> reps;
  fdt_shred_sets_group(arena, shreds, n, ok.data(), roots, codes, rep, reps);
  if (lanes) *lanes = reps.size();
  /* the representatives through the verifier: item = sig[64] | pub[32] | root[32], as fdgpu_fec_roots_verify */
  std::vector<int8_t> rc(std::max<size_t>(reps.size(), 1));
  Pipe p(v, rc.data());
  Chunk *c = nullptr;
  int r = p.next(&c);
  for (size_t k = 0; k < reps.size() && !r; k++) {
    const uint64_t i = reps[k];
    if (c->txns.size() == batch_max) {
      r = p.submit(*c);
      if (!r) r = p.next(&c);
      if (r) break;
    }
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
    c->items.push_back(k);
  }
  if (!r) r = p.submit(*c);
  if (!r) r = p.finish();
  if (r) return r;
  fdt_shred_sets_scatter(n, rep, reps, rc.data(), codes);
  return 0;
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

/* ---- precompiles ---- */

namespace {

struct rec_store {
  fdt_precompile_rec_t *recs;
  uint32_t cap, n = 0;
  void operator()(uint32_t j, uint32_t i, uint32_t sig_at, uint32_t pub_at, uint32_t msg_at, uint32_t msg_sz) {
    if (n < cap) recs[n] = {(uint16_t)j, (uint16_t)i, (uint16_t)sig_at, (uint16_t)pub_at, (uint16_t)msg_at, (uint16_t)msg_sz};
    n++;
  }
};

/* fn(i) for i in [0, n) on up to 16 threads, dealt in runs of 256 */
template <class Fn> void par_for(uint64_t n, Fn fn) {
  std::atomic<uint64_t> next{0};
  auto work = [&] {
    for (uint64_t b; (b = next.fetch_add(256)) < n;)
      for (uint64_t i = b; i < std::min(n, b + 256); i++) fn(i);
  };
  const unsigned hw = std::thread::hardware_concurrency();
  const uint64_t nt = std::min<uint64_t>({16, hw ? hw : 1, (n + 1023) / 1024});
  std::vector<std::thread> th;
  for (uint64_t t = 1; t < nt; t++) th.emplace_back(work);
  work();
  for (auto &t : th) t.join();
}

const fdgpu_precompile_info_t INFO_NONE = {0xFFFF, 0xFFFF, 0, 0, 0, {0, 0, 0, 0, 0, 0, 0}};

}  // namespace

extern "C" {

void fdt_precompile_walk(const uint8_t *payload, uint64_t sz, const void *txn, fdt_precompile_rec_t *recs, uint32_t rec_cap,
                         fdt_precompile_walk_t *out) {
  rec_store st{recs, recs ? rec_cap : 0u};
  fdt_precompile_walk_core(payload, sz, (const fdt_txn_t *)txn, st, out);
}

int fdt_precompile_verdict(const fdt_precompile_walk_t *walk, const fdt_precompile_rec_t *recs, const int8_t *ed_codes,
                           fdgpu_precompile_info_t *info) {
  fdgpu_precompile_info_t tmp;
  return fdt_precompile_verdict_core(
      walk->code, walk->instr_idx, walk->rec_idx, walk->ed_instr_cnt, walk->rec_cnt,
      [&](uint32_t k) { return (int)ed_codes[k]; },
      [&](uint32_t k) { return ((uint32_t)recs[k].instr_idx << 16) | recs[k].rec_idx; }, info ? info : &tmp);
}

int fdgpu_precompiles_verify(fdgpu_verifier_t v, const uint8_t *payloads, const uint64_t *off, const uint32_t *sz,
                             uint64_t n, uint64_t batch_max, int8_t *codes, fdgpu_precompile_info_t *info) {
  if (!v.submit || !v.poll || !codes || (n && (!payloads || !off || !sz)) || !batch_max) return FDGPU_ERR_INVAL;
  /* the walks first: a pass that counts each transaction's records, then one that stores them at their place */
  std::vector<fdt_precompile_walk_t> walk(std::max<uint64_t>(n, 1));
  std::vector<uint8_t> parsed(std::max<uint64_t>(n, 1));
  std::vector<uint64_t> rec0(n + 1, 0);
  auto one = [&](uint64_t i, fdt_precompile_rec_t *recs, uint32_t cap) {
    alignas(8) uint8_t txn_buf[FDT_TXN_MAX_SZ];
    const uint8_t *raw = payloads + off[i];
    parsed[i] = sz[i] <= FDT_TXN_MTU && fdt_txn_parse(raw, sz[i], txn_buf, nullptr) != 0;
    if (parsed[i]) fdt_precompile_walk(raw, sz[i], txn_buf, recs, cap, &walk[i]);
    else walk[i] = {FDGPU_CODE_PARSE_FAIL, 0, 0xFFFF, 0xFFFF, 0, 0};
  };
  par_for(n, [&](uint64_t i) { one(i, nullptr, 0); });
  for (uint64_t i = 0; i < n; i++) rec0[i + 1] = rec0[i] + walk[i].rec_cnt;
  const uint64_t total = rec0[n];
  std::vector<fdt_precompile_rec_t> recs(std::max<uint64_t>(total, 1));
  par_for(n, [&](uint64_t i) { if (walk[i].rec_cnt) one(i, recs.data() + rec0[i], walk[i].rec_cnt); });
  /* every record is one single-signature item: sig[64] | pub[32] | msg */
  std::vector<int8_t> ed(std::max<uint64_t>(total, 1));
  Pipe p(v, ed.data());
  Chunk *c = nullptr;
  int r = p.next(&c);
  for (uint64_t i = 0; i < n && !r; i++) {
    const uint8_t *raw = payloads + off[i];
    for (uint64_t k = rec0[i]; k < rec0[i + 1]; k++) {
      if (c->txns.size() == batch_max) {
        r = p.submit(*c);
        if (!r) r = p.next(&c);
        if (r) break;
      }
      const fdt_precompile_rec_t &q = recs[k];
      const uint32_t base = (uint32_t)c->arena.size();
      c->arena.insert(c->arena.end(), raw + q.sig_off, raw + q.sig_off + 64);
      c->arena.insert(c->arena.end(), raw + q.pub_off, raw + q.pub_off + 32);
      c->arena.insert(c->arena.end(), raw + q.msg_off, raw + q.msg_off + q.msg_sz);
      fdgpu_txn_t d;
      d.sig_off = base;
      d.pub_off = base + 64;
      d.msg_off = base + 96;
      d.msg_sz = q.msg_sz;
      d.sig_cnt = 1;
      c->txns.push_back(d);
      c->items.push_back(k);
    }
  }
  if (!r) r = p.submit(*c);
  if (!r) r = p.finish();
  if (r) return r;
  for (uint64_t i = 0; i < n; i++) {
    fdgpu_precompile_info_t tmp;
    fdgpu_precompile_info_t *o = info ? info + i : &tmp;
    if (!parsed[i]) { codes[i] = FDGPU_CODE_PARSE_FAIL; *o = INFO_NONE; continue; }
    codes[i] = (int8_t)fdt_precompile_verdict(&walk[i], recs.data() + rec0[i], ed.data() + rec0[i], o);
  }
  return 0;
}

int fdgpu_block_precompile_verify(fdgpu_engine_t *e, fdgpu_verifier_t v_host, const uint8_t *payloads, const uint64_t *off,
                                  const uint32_t *sz, uint64_t n_txn, uint64_t batch_txn_max, int8_t *codes,
                                  fdgpu_precompile_info_t *info) {
  if (!codes || !batch_txn_max || (n_txn && (!payloads || !off || !sz))) return FDGPU_ERR_INVAL;
  if (!e && (!v_host.submit || !v_host.poll)) return FDGPU_ERR_INVAL;
  /* the host's part: which transactions carry an Ed25519 instruction, and how many signature slots each needs */
  std::vector<uint32_t> cap(std::max<uint64_t>(n_txn, 1));
  std::vector<uint8_t> fwd(std::max<uint64_t>(n_txn, 1));
  par_for(n_txn, [&](uint64_t i) {
    alignas(8) uint8_t txn_buf[FDT_TXN_MAX_SZ];
    const uint8_t *raw = payloads + off[i];
    fwd[i] = 0;
    if (sz[i] > FDT_TXN_MTU || !fdt_txn_parse(raw, sz[i], txn_buf, nullptr)) {
      codes[i] = FDGPU_CODE_PARSE_FAIL;
      if (info) info[i] = INFO_NONE;
      return;
    }
    fdt_precompile_walk_t w;
    fdt_precompile_walk(raw, sz[i], txn_buf, nullptr, 0, &w);
    if (!w.ed_instr_cnt) {
      codes[i] = 0;
      if (info) info[i] = INFO_NONE;
      return;
    }
    fwd[i] = 1;
    cap[i] = w.rec_cnt;
  });
  std::vector<uint64_t> idx;
  for (uint64_t i = 0; i < n_txn; i++) if (fwd[i]) idx.push_back(i);
  if (idx.empty()) return 0;
  if (!e) {
    std::vector<uint64_t> o2(idx.size());
    std::vector<uint32_t> s2(idx.size());
    std::vector<int8_t> c2(idx.size());
    std::vector<fdgpu_precompile_info_t> i2(idx.size());
    for (size_t k = 0; k < idx.size(); k++) { o2[k] = off[idx[k]]; s2[k] = sz[idx[k]]; }
    const int r = fdgpu_precompiles_verify(v_host, payloads, o2.data(), s2.data(), idx.size(), batch_txn_max, c2.data(),
                                           i2.data());
    if (r) return r;
    for (size_t k = 0; k < idx.size(); k++) { codes[idx[k]] = c2[k]; if (info) info[idx[k]] = i2[k]; }
    return 0;
  }
  uint64_t txn_max = 0, sig_max = 0, arena_max = 0;
  if (fdgpu_poh_limits(e, &txn_max, &sig_max, &arena_max)) return FDGPU_ERR_INVAL;
  txn_max = std::min(txn_max, batch_txn_max);
  /* a batch: the forwarded payloads copied into an arena of the batch's own */
  struct PcChunk {
    std::vector<uint8_t> arena;
    std::vector<fdgpu_precompile_t> tx;
    std::vector<uint64_t> items;   /* caller's index of each transaction */
    uint64_t cap = 0;
    int64_t ticket = -1;
  } slot[2];
  int head = 0, cnt = 0;
  std::vector<int8_t> buf;
  std::vector<fdgpu_precompile_info_t> ibuf;
  auto drain_one = [&]() -> int {
    PcChunk &c = slot[head];
    buf.resize(std::max<size_t>(c.tx.size(), 1));
    ibuf.resize(std::max<size_t>(c.tx.size(), 1));
    const int r = fdgpu_poll_precompiles(e, c.ticket, buf.data(), ibuf.data(), 1);
    if (r != FDGPU_OK) return r < 0 ? r : FDGPU_ERR_DEVICE;
    for (size_t i = 0; i < c.items.size(); i++) { codes[c.items[i]] = buf[i]; if (info) info[c.items[i]] = ibuf[i]; }
    head ^= 1;
    cnt--;
    return 0;
  };
  auto next = [&](PcChunk **out) -> int {      /* the chunk to fill next (drains the oldest when both are busy) */
    if (cnt == 2) {
      const int r = drain_one();
      if (r) return r;
    }
    PcChunk &c = slot[(head + cnt) & 1];
    c.arena.clear(); c.tx.clear(); c.items.clear(); c.cap = 0;
    *out = &c;
    return 0;
  };
  auto submit = [&](PcChunk &c) -> int {
    if (c.tx.empty()) return 0;
    int64_t tk;
    while ((tk = fdgpu_submit_precompiles(e, c.arena.data(), c.arena.size(), c.tx.data(), c.tx.size())) == FDGPU_ERR_FULL) {
      if (!cnt) return FDGPU_ERR_FULL;
      const int r = drain_one();
      if (r) return r;
    }
    if (tk < 0) return (int)tk;
    c.ticket = tk;
    cnt++;
    return 0;
  };
  PcChunk *c = nullptr;
  int r = next(&c);
  for (size_t k = 0; k < idx.size() && !r; k++) {
    const uint64_t i = idx[k];
    if (cap[i] > sig_max || sz[i] > arena_max) { r = FDGPU_ERR_INVAL; break; }   /* one transaction no batch can hold */
    if (c->tx.size() == txn_max || c->cap + cap[i] > sig_max || c->arena.size() + sz[i] > arena_max) {
      r = submit(*c);
      if (!r) r = next(&c);
      if (r) break;
    }
    fdgpu_precompile_t d;
    d.off = (uint32_t)c->arena.size();
    d.sz = sz[i];
    d.sig_cap = cap[i];
    c->arena.insert(c->arena.end(), payloads + off[i], payloads + off[i] + sz[i]);
    c->tx.push_back(d);
    c->items.push_back(i);
    c->cap += cap[i];
  }
  if (!r) r = submit(*c);
  while (cnt) {                                /* on an error too: no batch is left in the ring */
    const int d = drain_one();
    if (d) return r ? r : d;
  }
  return r;
}

}  // extern "C"

/* ---- secp256k1 precompile ---- */

namespace {

int k1_record(const uint8_t *payload, const fdt_precompile_rec_t &q) {
  fdt_keccak_plain_reader r{payload};
  return fdt_secp256k1_record_core(r, q.msg_off, q.msg_sz, q.sig_off, q.pub_off);
}

void be32_to_u256(fdt_u256 &a, const uint8_t *b) {
  fdt_keccak_plain_reader r{b};
  fdt_u256_load_be(a, r, 0);
}

void u256_to_be32(uint8_t *b, const fdt_u256 &a) {
  for (int i = 0; i < 8; i++)
    for (int k = 0; k < 4; k++) b[4 * (7 - i) + k] = (uint8_t)(a.v[i] >> (8 * (3 - k)));
}

}  // namespace

extern "C" {

void fdt_keccak256(const uint8_t *msg, uint64_t sz, uint8_t *out) { fdt_keccak256_core(msg, sz, out); }

int fdt_secp256k1_recover(const uint8_t *hash, const uint8_t *sig, int recid, uint8_t *key) {
  fdt_u256 h, r, s, x, y;
  be32_to_u256(h, hash);
  be32_to_u256(r, sig);
  be32_to_u256(s, sig + 32);
  const int rc = fdt_secp256k1_recover_core(h, r, s, (uint32_t)recid, x, y);
  u256_to_be32(key, x);
  u256_to_be32(key + 32, y);
  return rc;
}

void fdt_secp256k1_walk(const uint8_t *payload, uint64_t sz, const void *txn, uint32_t flags, fdt_precompile_rec_t *recs,
                        uint32_t rec_cap, fdt_precompile_walk_t *out) {
  rec_store st{recs, recs ? rec_cap : 0u};
  fdt_secp256k1_walk_core(payload, sz, (const fdt_txn_t *)txn, flags, st, out);
}

int fdt_secp256k1_record(const uint8_t *payload, uint64_t sz, const fdt_precompile_rec_t *rec) {
  (void)sz;
  return k1_record(payload, *rec);
}

int fdt_secp256k1_verdict(const fdt_precompile_walk_t *walk, const fdt_precompile_rec_t *recs, const int8_t *codes,
                          fdgpu_precompile_info_t *info) {
  fdgpu_precompile_info_t tmp;
  return fdt_secp256k1_verdict_core(
      walk->code, walk->instr_idx, walk->rec_idx, walk->ed_instr_cnt, walk->rec_cnt,
      [&](uint32_t k) { return (int)codes[k]; },
      [&](uint32_t k) { return ((uint32_t)recs[k].instr_idx << 16) | recs[k].rec_idx; }, info ? info : &tmp);
}

int fdgpu_secp256k1_verify_host(const uint8_t *payloads, const uint64_t *off, const uint32_t *sz, uint64_t n, uint32_t flags,
                                int8_t *codes, fdgpu_precompile_info_t *info) {
  if (!codes || (n && (!payloads || !off || !sz))) return FDGPU_ERR_INVAL;
  /* the walks first, then the records -- the expensive part -- dealt over the threads one by one */
  std::vector<fdt_precompile_walk_t> walk(std::max<uint64_t>(n, 1));
  std::vector<uint8_t> parsed(std::max<uint64_t>(n, 1));
  std::vector<uint64_t> rec0(n + 1, 0);
  auto one = [&](uint64_t i, fdt_precompile_rec_t *recs, uint32_t cap) {
    alignas(8) uint8_t txn_buf[FDT_TXN_MAX_SZ];
    const uint8_t *raw = payloads + off[i];
    parsed[i] = sz[i] <= FDT_TXN_MTU && fdt_txn_parse(raw, sz[i], txn_buf, nullptr) != 0;
    if (parsed[i]) fdt_secp256k1_walk(raw, sz[i], txn_buf, flags, recs, cap, &walk[i]);
    else walk[i] = {FDGPU_CODE_PARSE_FAIL, 0, 0xFFFF, 0xFFFF, 0, 0};
  };
  par_for(n, [&](uint64_t i) { one(i, nullptr, 0); });
  for (uint64_t i = 0; i < n; i++) rec0[i + 1] = rec0[i] + walk[i].rec_cnt;
  const uint64_t total = rec0[n];
  std::vector<fdt_precompile_rec_t> recs(std::max<uint64_t>(total, 1));
  std::vector<uint32_t> owner(std::max<uint64_t>(total, 1));
  par_for(n, [&](uint64_t i) {
    if (!walk[i].rec_cnt) return;
    one(i, recs.data() + rec0[i], walk[i].rec_cnt);
    for (uint64_t k = rec0[i]; k < rec0[i + 1]; k++) owner[k] = (uint32_t)i;
  });
  std::vector<int8_t> rc(std::max<uint64_t>(total, 1));
  {
    std::atomic<uint64_t> next{0};
    auto work = [&] {
      for (uint64_t k; (k = next.fetch_add(1)) < total;) rc[k] = (int8_t)k1_record(payloads + off[owner[k]], recs[k]);
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const uint64_t nt = std::min<uint64_t>({16, hw ? hw : 1, total});
    std::vector<std::thread> th;
    for (uint64_t t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
  }
  for (uint64_t i = 0; i < n; i++) {
    fdgpu_precompile_info_t tmp;
    fdgpu_precompile_info_t *o = info ? info + i : &tmp;
    if (!parsed[i]) { codes[i] = FDGPU_CODE_PARSE_FAIL; *o = INFO_NONE; continue; }
    codes[i] = (int8_t)fdt_secp256k1_verdict(&walk[i], recs.data() + rec0[i], rc.data() + rec0[i], o);
  }
  return 0;
}

int fdgpu_block_secp256k1_verify(fdgpu_engine_t *e, const uint8_t *payloads, const uint64_t *off, const uint32_t *sz,
                                 uint64_t n_txn, uint32_t flags, uint64_t batch_txn_max, int8_t *codes,
                                 fdgpu_precompile_info_t *info) {
  if (!codes || !batch_txn_max || (n_txn && (!payloads || !off || !sz))) return FDGPU_ERR_INVAL;
  /* the host's part: which transactions carry a secp256k1 instruction, and how many record slots each needs */
  std::vector<uint32_t> cap(std::max<uint64_t>(n_txn, 1));
  std::vector<uint8_t> fwd(std::max<uint64_t>(n_txn, 1));
  par_for(n_txn, [&](uint64_t i) {
    alignas(8) uint8_t txn_buf[FDT_TXN_MAX_SZ];
    const uint8_t *raw = payloads + off[i];
    fwd[i] = 0;
    if (sz[i] > FDT_TXN_MTU || !fdt_txn_parse(raw, sz[i], txn_buf, nullptr)) {
      codes[i] = FDGPU_CODE_PARSE_FAIL;
      if (info) info[i] = INFO_NONE;
      return;
    }
    fdt_precompile_walk_t w;
    fdt_secp256k1_walk(raw, sz[i], txn_buf, flags, nullptr, 0, &w);
    if (!w.ed_instr_cnt) {
      codes[i] = 0;
      if (info) info[i] = INFO_NONE;
      return;
    }
    fwd[i] = 1;
    cap[i] = w.rec_cnt;
  });
  std::vector<uint64_t> idx;
  for (uint64_t i = 0; i < n_txn; i++) if (fwd[i]) idx.push_back(i);
  if (idx.empty()) return 0;
  if (!e) {
    std::vector<uint64_t> o2(idx.size());
    std::vector<uint32_t> s2(idx.size());
    std::vector<int8_t> c2(idx.size());
    std::vector<fdgpu_precompile_info_t> i2(idx.size());
    for (size_t k = 0; k < idx.size(); k++) { o2[k] = off[idx[k]]; s2[k] = sz[idx[k]]; }
    const int r = fdgpu_secp256k1_verify_host(payloads, o2.data(), s2.data(), idx.size(), flags, c2.data(), i2.data());
    if (r) return r;
    for (size_t k = 0; k < idx.size(); k++) { codes[idx[k]] = c2[k]; if (info) info[idx[k]] = i2[k]; }
    return 0;
  }
  uint64_t txn_max = 0, sig_max = 0, arena_max = 0;
  if (fdgpu_poh_limits(e, &txn_max, &sig_max, &arena_max)) return FDGPU_ERR_INVAL;
  txn_max = std::min(txn_max, batch_txn_max);
  /* a batch: the forwarded payloads copied into an arena of the batch's own; two in flight */
  struct K1Chunk {
    std::vector<uint8_t> arena;
    std::vector<fdgpu_precompile_t> tx;
    std::vector<uint64_t> items;   /* caller's index of each transaction */
    uint64_t cap = 0;
    int64_t ticket = -1;
  } slot[2];
  int head = 0, cnt = 0;
  std::vector<int8_t> buf;
  std::vector<fdgpu_precompile_info_t> ibuf;
  auto drain_one = [&]() -> int {
    K1Chunk &c = slot[head];
    buf.resize(std::max<size_t>(c.tx.size(), 1));
    ibuf.resize(std::max<size_t>(c.tx.size(), 1));
    const int r = fdgpu_poll_secp256k1(e, c.ticket, buf.data(), ibuf.data(), 1);
    if (r != FDGPU_OK) return r < 0 ? r : FDGPU_ERR_DEVICE;
    for (size_t i = 0; i < c.items.size(); i++) { codes[c.items[i]] = buf[i]; if (info) info[c.items[i]] = ibuf[i]; }
    head ^= 1;
    cnt--;
    return 0;
  };
  auto next = [&](K1Chunk **out) -> int {
    if (cnt == 2) {
      const int r = drain_one();
      if (r) return r;
    }
    K1Chunk &c = slot[(head + cnt) & 1];
    c.arena.clear(); c.tx.clear(); c.items.clear(); c.cap = 0;
    *out = &c;
    return 0;
  };
  auto submit = [&](K1Chunk &c) -> int {
    if (c.tx.empty()) return 0;
    int64_t tk;
    while ((tk = fdgpu_submit_secp256k1(e, c.arena.data(), c.arena.size(), c.tx.data(), c.tx.size(), flags)) == FDGPU_ERR_FULL) {
      if (!cnt) return FDGPU_ERR_FULL;
      const int r = drain_one();
      if (r) return r;
    }
    if (tk < 0) return (int)tk;
    c.ticket = tk;
    cnt++;
    return 0;
  };
  K1Chunk *c = nullptr;
  int r = next(&c);
  for (size_t k = 0; k < idx.size() && !r; k++) {
    const uint64_t i = idx[k];
    if (cap[i] > sig_max || sz[i] > arena_max) { r = FDGPU_ERR_INVAL; break; }   /* one transaction no batch can hold */
    if (c->tx.size() == txn_max || c->cap + cap[i] > sig_max || c->arena.size() + sz[i] > arena_max) {
      r = submit(*c);
      if (!r) r = next(&c);
      if (r) break;
    }
    fdgpu_precompile_t d;
    d.off = (uint32_t)c->arena.size();
    d.sz = sz[i];
    d.sig_cap = cap[i];
    c->arena.insert(c->arena.end(), payloads + off[i], payloads + off[i] + sz[i]);
    c->tx.push_back(d);
    c->items.push_back(i);
    c->cap += cap[i];
  }
  if (!r) r = submit(*c);
  while (cnt) {                                /* on an error too: no batch is left in the ring */
    const int d = drain_one();
    if (d) return r ? r : d;
  }
  return r;
}

int fdgpu_precompile_merge(int ed_code, const fdgpu_precompile_info_t *ed_info, int k1_code,
                           const fdgpu_precompile_info_t *k1_info, fdgpu_precompile_info_t *out) {
  fdgpu_precompile_info_t tmp;
  fdgpu_precompile_info_t *o = out ? out : &tmp;
  const fdgpu_precompile_info_t a = ed_info ? *ed_info : INFO_NONE, b = k1_info ? *k1_info : INFO_NONE;
  *o = INFO_NONE;
  if (ed_code == FDGPU_CODE_PARSE_FAIL || k1_code == FDGPU_CODE_PARSE_FAIL) return FDGPU_CODE_PARSE_FAIL;
  if (ed_code == FDGPU_CODE_PRECOMPILE_CAP || k1_code == FDGPU_CODE_PRECOMPILE_CAP) return FDGPU_CODE_PRECOMPILE_CAP;
  /* the first failing instruction of either program (fd_executor.c:255-267); an instruction has one program, so
     two failures never share an index */
  const int which = !ed_code && !k1_code ? 0 : !k1_code ? 1 : !ed_code ? 2 : a.instr_idx <= b.instr_idx ? 1 : 2;
  const fdgpu_precompile_info_t &w = which == 2 ? b : a;
  if (which) { o->instr_idx = w.instr_idx; o->rec_idx = w.rec_idx; o->ed_code = w.ed_code; }
  o->ed_instr_cnt = (uint16_t)(a.ed_instr_cnt + b.ed_instr_cnt);
  o->sig_cnt = (uint16_t)(a.sig_cnt + b.sig_cnt);
  o->_pad[0] = (uint8_t)which;
  return which == 0 ? 0 : which == 1 ? ed_code : k1_code;
}

int fdgpu_block_precompile_verify_all(fdgpu_engine_t *e, fdgpu_verifier_t v_host, const uint8_t *payloads, const uint64_t *off,
                                      const uint32_t *sz, uint64_t n_txn, uint32_t flags, uint64_t batch_txn_max,
                                      int8_t *codes, fdgpu_precompile_info_t *info) {
  if (!codes) return FDGPU_ERR_INVAL;
  std::vector<int8_t> c1(std::max<uint64_t>(n_txn, 1)), c2(std::max<uint64_t>(n_txn, 1));
  std::vector<fdgpu_precompile_info_t> i1(std::max<uint64_t>(n_txn, 1)), i2(std::max<uint64_t>(n_txn, 1));
  int r = fdgpu_block_precompile_verify(e, v_host, payloads, off, sz, n_txn, batch_txn_max, c1.data(), i1.data());
  if (!r) r = fdgpu_block_secp256k1_verify(e, payloads, off, sz, n_txn, flags, batch_txn_max, c2.data(), i2.data());
  if (r) return r;
  for (uint64_t i = 0; i < n_txn; i++)
    codes[i] = (int8_t)fdgpu_precompile_merge(c1[i], &i1[i], c2[i], &i2[i], info ? info + i : nullptr);
  return 0;
}

}  // extern "C"
