/* fdgpu_sync.cpp -- the reference's synchronous per-call API (fd_ed25519.h:96-101,124-130) on one process-wide engine
   on device 0.  A call is one GPU round trip: about a millisecond, the lifetime of the verify kernel's single wave,
   not the CPU's ~30 us (bench.py `sync_*` lines).

   Calls from concurrent threads are coalesced (group commit): a caller that finds no batch in flight becomes the
   leader, takes every call queued so far as one batch (one txn per call) and verifies it; calls arriving meanwhile
   queue for the next leader.  A lone caller pays one round trip, N concurrent callers share theirs, so throughput
   grows with the number of callers instead of serialising on a lock.  The caller's current HIP device is saved and
   restored.

   A call whose message does not fit one batch arena (32-bit offsets: about 2 GB) is verified alone: its k = SHA-512(R
   || A || M) is hashed on the device in arena-sized pieces of M (fdgpu_sha512_stream_kernel), then the verify runs
   from those digests -- the reference hashes any msg_sz (fd_ed25519_user.c:205-207), so size is never an error
   here.  FDGPU_SYNC_ARENA_MAX=<bytes> lowers that limit (tests reach the path with small messages).

   The reference API has no error channel besides the verify codes, and it never answers a good signature with an
   error.  So an engine failure (no device, a HIP error) aborts the process by default, with the reason on stderr: a
   transient GPU fault must not turn valid transactions or blocks into rejected ones (replay's fd_executor_txn_verify,
   the shred FEC-root checks).  A caller that prefers to reject instead sets FDGPU_SYNC_FAIL_CLOSED=1: every call of
   the failed batch then returns FD_ED25519_ERR_SIG and fdgpu_sync_errors() counts the event (fdgpu_last_error() of
   the failing thread says why).  FDGPU_SYNC_DEVICE=<n> puts the engine on device n (default 0). */
#include <algorithm>
#include <condition_variable>

#include "fdgpu_engine.h"

using namespace fdgpu;

namespace {

/* The synchronous API's environment switches, beside the engine's Env (fdgpu_engine.h); constructing one reads them */
struct SyncEnv {
  uint64_t arena_max = (uint64_t)env_num(getenv("FDGPU_SYNC_ARENA_MAX"), 0, 0);   /* load: unset; see SYNC_ARENA_MAX */
  bool fail_closed = env_is(getenv("FDGPU_SYNC_FAIL_CLOSED"), '1');   /* each failure: off, abort; 1: reject the calls */
  bool pair = !env_is(getenv("FDGPU_SYNC_PAIR"), '0');   /* each (re)open: on; 0: no auto pair / spread flags */
  int device = (int)env_num(getenv("FDGPU_SYNC_DEVICE"), 0);   /* each (re)open: device 0 */
};

struct SyncReq {
  const uint8_t *msg, *sigs, *pubs;
  uint64_t msg_sz;
  uint32_t n;
  int code = 0;
  bool done = false;
};

struct SyncState {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<SyncReq *> pending;
  bool leader = false;
  fdgpu_engine_t *eng = nullptr;
  std::vector<uint8_t> arena;
  std::vector<fdgpu_txn_t> txns;
  std::vector<int8_t> codes;
  std::atomic<uint64_t> errors{0}, calls{0}, batches{0};
};

SyncState &sync_state() {
  /* leaked on purpose: no destructor runs at exit, after the HIP runtime may already be gone, or while a caller
     thread still waits */
  static SyncState *st = new SyncState;
  return *st;
}

constexpr uint64_t SYNC_BATCH_MAX = 4096;    /* calls per coalesced batch */
/* arena bytes of one coalesced batch: the engine's arena is opened at twice the batch's need (room to grow) and must
   stay within 32-bit offsets (fdgpu_engine_open), so a batch holds at most half of that; a single call needing more
   cannot run on the engine at all.  The override, read when the library is loaded, only lowers the limit. */
constexpr uint64_t SYNC_ARENA_LIMIT = (0xFFFFFFF0ull - FDGPU_ARENA_SLACK) / 2;
const uint64_t SYNC_ARENA_MAX = [] {
  const uint64_t m = SyncEnv().arena_max;
  return m >= 1024 && m < SYNC_ARENA_LIMIT ? m : SYNC_ARENA_LIMIT;
}();
inline uint64_t sync_need(uint64_t msg_sz, uint32_t n) { return 96ull * n + msg_sz; }

void sync_failed(SyncState &st, const char *what) {
  st.errors.fetch_add(1, std::memory_order_relaxed);
  if (!SyncEnv().fail_closed) {
    fprintf(stderr, "fd_ed25519_gpu: %s: %s (FDGPU_SYNC_FAIL_CLOSED=1 rejects the calls instead)\n", what,
            fdgpu_last_error());
    abort();
  }
}

/* the coalesced batch's engine, (re)opened for a batch needing `need` arena bytes (0: as it is) */
bool sync_open(SyncState &st, uint64_t need) {
  if (!st.eng || need > st.eng->cfg.max_arena) {
    if (st.eng) fdgpu_engine_close(st.eng);
    const SyncEnv now;
    fdgpu_cfg_t cfg{};
    cfg.max_txn = SYNC_BATCH_MAX; cfg.max_sig = SYNC_BATCH_MAX * 16; cfg.ring_depth = 1;
    /* a call's batch is small (one txn per concurrent caller): the two-lane kernel's shorter wave is the call's
       latency (SyncEnv::pair) */
    cfg.flags = now.pair ? FDGPU_FLAG_PAIR_AUTO | FDGPU_FLAG_SPREAD_AUTO : 0u;
    cfg.max_arena = std::min<uint64_t>(std::max<uint64_t>(SYNC_BATCH_MAX * (96 * 16 + 1232), need * 2),
                                       2 * SYNC_ARENA_LIMIT);
    st.eng = fdgpu_engine_open(now.device, &cfg);
    if (!st.eng) return false;
  }
  return true;
}

/* One call whose message exceeds a batch arena: k_i = SHA-512(R_i || A_i || M) for its n signatures on the device, a
   piece of M (at most SYNC_ARENA_MAX bytes) per launch of fdgpu_sha512_stream_kernel, then the verify from those
   digests and the batch_single_msg combine -- the same code a batch would give it.  Buffers are the call's own (a
   rare path). */
bool sync_run_prehashed(SyncState &st, SyncReq &r) {
  if (!sync_open(st, 0)) return false;
  fdgpu_engine_t *e = st.eng;
  HIPCHK(hipSetDevice(e->device), false);
  const uint32_t n = r.n;
  const uint64_t sig_at = 0, pub_at = 64ull * n, st_at = (pub_at + 32ull * n + 63) & ~63ull;
  const uint64_t arena_sz = st_at + 64ull * n;
  const uint64_t piece = std::max<uint64_t>(256, SYNC_ARENA_MAX & ~127ull);
  const uint64_t per_launch = piece / 128 - 1;            /* blocks whose message bytes fit one piece */
  hipStream_t s = e->compute;
  DevBuf<uint8_t> d_arena, d_m, d_ra, d_codes;
  DevBuf<fdgpu_sig_desc_t> d_sigs;
  DevBuf<fdgpu_txn_desc_t> d_txn;
  DevBuf<uint32_t> d_ws;
  /* on every return the stream is drained before the buffers above go */
  struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{s};
  if (d_arena.alloc(arena_sz + FDGPU_ARENA_SLACK) != hipSuccess || d_m.alloc(piece) != hipSuccess ||
      d_ra.alloc(64ull * n) != hipSuccess || d_codes.alloc(2ull * n + 32) != hipSuccess ||
      d_sigs.alloc(n * sizeof(fdgpu_sig_desc_t)) != hipSuccess || d_txn.alloc(sizeof(fdgpu_txn_desc_t)) != hipSuccess ||
      d_ws.alloc(fdgpu_ws_bytes(n)) != hipSuccess) {
    set_err("prehashed call: device allocation");
    return false;
  }
  std::vector<uint8_t> h_arena(arena_sz, 0), h_ra(64ull * n);
  std::vector<fdgpu_sig_desc_t> h_sigs(n);
  for (uint32_t i = 0; i < n; i++) {
    memcpy(h_arena.data() + sig_at + 64ull * i, r.sigs + 64ull * i, 64);
    memcpy(h_arena.data() + pub_at + 32ull * i, r.pubs + 32ull * i, 32);
    memcpy(h_ra.data() + 64ull * i, r.sigs + 64ull * i, 32);        /* R */
    memcpy(h_ra.data() + 64ull * i + 32, r.pubs + 32ull * i, 32);   /* A */
    h_sigs[i] = fdgpu_sig_desc_t{(uint32_t)(st_at + 64ull * i), 0u, (uint32_t)(sig_at + 64ull * i),
                                 (uint32_t)(pub_at + 32ull * i)};
  }
  const fdgpu_txn_desc_t h_txn{0u, n};
  if (hipMemcpyAsync(d_arena, h_arena.data(), arena_sz, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(d_ra, h_ra.data(), 64ull * n, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(d_sigs, h_sigs.data(), n * sizeof(fdgpu_sig_desc_t), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(d_txn, &h_txn, sizeof h_txn, hipMemcpyHostToDevice, s) != hipSuccess) {
    set_err("prehashed call: upload");
    return false;
  }
  const uint64_t total = fdgpu_sha512_stream_blocks(r.msg_sz);
  bool hashed = true;
  for (uint64_t b0 = 0; b0 < total && hashed; b0 += per_launch) {
    const uint64_t b1 = std::min(total, b0 + per_launch);
    /* the message bytes of blocks [b0, b1): M[128 b0 - 64, 128 b1 + 64) within M */
    const uint64_t m0 = b0 ? 128 * b0 - 64 : 0, m1 = std::min<uint64_t>(r.msg_sz, 128 * b1 + 64);
    const uint64_t mlen = m1 > m0 ? m1 - m0 : 0;
    hashed = (!mlen || hipMemcpyAsync(d_m, r.msg + m0, mlen, hipMemcpyHostToDevice, s) == hipSuccess) &&
             fdgpu_launch_sha512_stream(d_m, m0, mlen, r.msg_sz, b0, (uint32_t)(b1 - b0), d_ra,
                                        (uint64_t *)(d_arena + st_at), n, s) == hipSuccess &&
             hipStreamSynchronize(s) == hipSuccess;              /* the piece buffer is reused next */
  }
  if (!hashed) { set_err("prehashed call: hashing"); return false; }
  int8_t *codes = (int8_t *)d_codes.p, code = 0;
  if (fdgpu_launch_verify_prehashed(d_arena, d_sigs, n, e->d_btab, d_ws, codes, kflags(e), s) != hipSuccess ||
      fdgpu_launch_combine(d_txn, 1, codes, codes + n + 16, nullptr, s) != hipSuccess ||
      hipMemcpyAsync(&code, codes + n + 16, 1, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    set_err("prehashed call: verify");
    return false;
  }
  r.code = code;
  return true;
}

/* the batch's calls into the arena, one txn each, verified on the engine */
bool sync_fill_run(SyncState &st, const std::vector<SyncReq *> &batch, uint64_t need) {
  st.arena.resize(need);
  st.txns.resize(batch.size());
  st.codes.resize(batch.size());
  uint64_t o = 0;
  for (size_t k = 0; k < batch.size(); k++) {
    const SyncReq &r = *batch[k];
    fdgpu_txn_t &t = st.txns[k];
    t.sig_off = (uint32_t)o; memcpy(st.arena.data() + o, r.sigs, 64ull * r.n); o += 64ull * r.n;
    t.pub_off = (uint32_t)o; memcpy(st.arena.data() + o, r.pubs, 32ull * r.n); o += 32ull * r.n;
    t.msg_off = (uint32_t)o; if (r.msg_sz) memcpy(st.arena.data() + o, r.msg, r.msg_sz); o += r.msg_sz;
    t.msg_sz = (uint32_t)r.msg_sz; t.sig_cnt = r.n;
  }
  const int64_t tk = fdgpu_submit(st.eng, st.arena.data(), need, st.txns.data(), batch.size());
  if (tk < 0) return false;
  if (fdgpu_poll(st.eng, tk, st.codes.data(), 1) != FDGPU_OK) return false;
  for (size_t k = 0; k < batch.size(); k++) batch[k]->code = st.codes[k];
  return true;
}

/* the leader's batch: returns false on an engine failure */
bool sync_run(SyncState &st, const std::vector<SyncReq *> &batch) {
  uint64_t need = 0;
  for (const SyncReq *r : batch) need += sync_need(r->msg_sz, r->n);
  if (need > SYNC_ARENA_MAX) {
    if (batch.size() == 1) return sync_run_prehashed(st, *batch[0]);    /* a call alone: its message in pieces */
    set_err("a batch needs %llu arena bytes (at most %llu)", (unsigned long long)need,
            (unsigned long long)SYNC_ARENA_MAX);
    return false;
  }
  if (!sync_open(st, need)) return false;
  return sync_fill_run(st, batch, need);
}

int sync_verify(const uint8_t *msg, uint64_t msg_sz, const uint8_t *sigs, const uint8_t *pubs, uint32_t n) {
  if (n == 0 || n > 16) return FD_ED25519_ERR_SIG;            /* fd_ed25519_user.c:238-241 */
  SyncState &st = sync_state();
  st.calls.fetch_add(1, std::memory_order_relaxed);
  SyncReq req{msg, sigs, pubs, msg_sz, n};
  std::unique_lock<std::mutex> lk(st.mu);
  st.pending.push_back(&req);
  while (!req.done) {
    if (st.leader) { st.cv.wait(lk); continue; }
    st.leader = true;                          /* this thread verifies everything queued so far */
    std::vector<SyncReq *> batch;
    /* as many queued calls as fit one batch's arena; a call that fits no arena is taken alone (its message is then
       hashed in pieces) */
    size_t take = 0;
    uint64_t need = 0;
    while (take < st.pending.size() && take < SYNC_BATCH_MAX) {
      const uint64_t c = sync_need(st.pending[take]->msg_sz, st.pending[take]->n);
      if (take && need + c > SYNC_ARENA_MAX) break;
      need += c;
      take++;
    }
    batch.assign(st.pending.begin(), st.pending.begin() + (long)take);
    st.pending.erase(st.pending.begin(), st.pending.begin() + (long)take);
    lk.unlock();
    int prev_dev = -1;
    if (hipGetDevice(&prev_dev) != hipSuccess) prev_dev = -1;
    const bool ok = sync_run(st, batch);
    if (prev_dev >= 0) (void)hipSetDevice(prev_dev);
    if (!ok) {
      sync_failed(st, "verify batch failed");
      for (SyncReq *r : batch) r->code = FD_ED25519_ERR_SIG;   /* fail closed */
      if (st.eng) { fdgpu_engine_close(st.eng); st.eng = nullptr; }   /* reopened by the next batch */
    }
    st.batches.fetch_add(1, std::memory_order_relaxed);
    lk.lock();
    for (SyncReq *r : batch) r->done = true;
    st.leader = false;
    st.cv.notify_all();
  }
  return req.code;
}

}  // namespace

extern "C" {

int fd_ed25519_verify(uint8_t const msg[], uint64_t msg_sz, uint8_t const sig[64], uint8_t const public_key[32],
                      fd_sha512_t *sha) {
  (void)sha;
  return sync_verify(msg, msg_sz, sig, public_key, 1);
}

int fd_ed25519_verify_batch_single_msg(uint8_t const msg[], uint64_t const msg_sz, uint8_t const signatures[64],
                                       uint8_t const pubkeys[32], fd_sha512_t *shas[1], uint8_t const batch_sz) {
  (void)shas;
  return sync_verify(msg, msg_sz, signatures, pubkeys, batch_sz);
}

int fdgpu_ed25519_verify(uint8_t const msg[], uint64_t msg_sz, uint8_t const sig[64], uint8_t const public_key[32]) {
  return sync_verify(msg, msg_sz, sig, public_key, 1);
}

int fdgpu_ed25519_verify_batch_single_msg(uint8_t const msg[], uint64_t msg_sz, uint8_t const signatures[64],
                                          uint8_t const pubkeys[32], uint8_t batch_sz) {
  return sync_verify(msg, msg_sz, signatures, pubkeys, batch_sz);
}

void fdgpu_sync_stats(uint64_t *calls, uint64_t *batches, uint64_t *errors) {
  SyncState &st = sync_state();
  if (calls) *calls = st.calls.load(std::memory_order_relaxed);
  if (batches) *batches = st.batches.load(std::memory_order_relaxed);
  if (errors) *errors = st.errors.load(std::memory_order_relaxed);
}

uint64_t fdgpu_sync_errors(void) { return sync_state().errors.load(std::memory_order_relaxed); }

char const *fd_ed25519_strerror(int err) {
  switch (err) {
    case FD_ED25519_SUCCESS: return "success";
    case FD_ED25519_ERR_SIG: return "bad signature";
    case FD_ED25519_ERR_PUBKEY: return "bad public key";
    case FD_ED25519_ERR_MSG: return "bad message";
    default: break;
  }
  return "unknown";
}

}  // extern "C"
