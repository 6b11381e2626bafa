/* secp256k1_san.cpp -- the host side of the secp256k1 precompile (firedancer_amd/csrc/fdt_secp256k1.h and
   fdt_keccak256.h, the source both the host library and the GPU kernels compile) behind fdt_parse_core, under the
   sanitizers, as a program of its own:

     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include \
         tools/secp256k1_san.cpp -o secp256k1_san
     ./secp256k1_san cases.bin vectors.bin <random_cnt> <record_cnt>

   cases.bin: records [u32 size][u8 flags][i8 expected verdict, or -64 when the payload does not parse][i8 expected
   record code][u16 expected record count][size bytes].  vectors.bin: records [u8 kind]; kind 1: [u32 size][size
   bytes][32 digest bytes] for the Keccak, kind 2: [97 bytes hash | r | s | recid][i8 code][64 key bytes] for the
   recover.  Then random_cnt buffers: mutations (one to three bytes, biased towards the instruction data; now and
   then a truncation) of the cases that parse, walked with both flag settings; the first record_cnt records they emit
   are checked too (a check is two hashes and a recover, slow under the sanitizers).  Every payload, every parsed
   fd_txn_t, every record array and every message lives in a heap allocation of exactly its size, so a read or write
   past it is an error the sanitizer reports.  tests/test_secp256k1.py builds and runs it. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../firedancer_amd/csrc/fdt_secp256k1.h"

struct store {
  fdt_precompile_rec_t *recs;
  uint32_t cap, n;
  void operator()(uint32_t j, uint32_t i, uint32_t s, uint32_t a, uint32_t m, uint32_t ms) {
    if (n < cap) recs[n] = {(uint16_t)j, (uint16_t)i, (uint16_t)s, (uint16_t)a, (uint16_t)m, (uint16_t)ms};
    n++;
  }
};
struct count {
  void operator()(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {}
};

static unsigned long g_budget = 0, g_checked = 0;

/* -> the verdict (or -64); *rec_cnt the records emitted, *rec_code the failing record's code.  check_all: every
   record is checked; else only while the budget lasts, the rest pass. */
static int run(const std::vector<uint8_t> &v, uint32_t flags, bool check_all, uint32_t *rec_cnt, int *rec_code) {
  uint8_t *p = (uint8_t *)malloc(v.size() ? v.size() : 1);    /* exact size: no slack behind the payload */
  if (!p) abort();
  if (!v.empty()) memcpy(p, v.data(), v.size());
  uint64_t fail = 0;
  *rec_cnt = 0;
  *rec_code = 0;
  const uint64_t fp = fdt_parse_core(p, v.size(), nullptr, &fail);
  int code = FDGPU_CODE_PARSE_FAIL;
  if (fp) {
    if (fp > FDT_TXN_MAX_SZ) abort();
    fdt_txn_t *t = (fdt_txn_t *)malloc(fp);                    /* exact size: the footprint the parser reported */
    if (!t || fdt_parse_core(p, v.size(), t, &fail) != fp) abort();
    fdt_precompile_walk_t w, w2;
    count c;
    fdt_secp256k1_walk_core(p, v.size(), t, flags, c, &w);
    if (w.rec_cnt > fdt_secp256k1_sig_bound(v.size())) abort();
    fdt_precompile_rec_t *recs = (fdt_precompile_rec_t *)malloc(w.rec_cnt ? w.rec_cnt * sizeof *recs : 1);
    int8_t *codes = (int8_t *)calloc(w.rec_cnt ? w.rec_cnt : 1, 1);
    if (!recs || !codes) abort();
    store st{recs, w.rec_cnt, 0};
    fdt_secp256k1_walk_core(p, v.size(), t, flags, st, &w2);
    if (st.n != w.rec_cnt || w2.rec_cnt != w.rec_cnt || w2.code != w.code || w2.instr_idx != w.instr_idx ||
        w2.rec_idx != w.rec_idx || w2.ed_instr_cnt != w.ed_instr_cnt)
      abort();
    for (uint32_t k = 0; k < w.rec_cnt; k++) {
      const fdt_precompile_rec_t &q = recs[k];
      if ((uint64_t)q.sig_off + 65 > v.size() || (uint64_t)q.pub_off + 20 > v.size() ||
          (uint64_t)q.msg_off + q.msg_sz > v.size() || q.instr_idx >= t->instr_cnt)
        abort();
      if (check_all || g_checked < g_budget) {
        fdt_keccak_plain_reader r{p};
        codes[k] = (int8_t)fdt_secp256k1_record_core(r, q.msg_off, q.msg_sz, q.sig_off, q.pub_off);
        if (codes[k] > 0 || codes[k] < FDT_SECP256K1_ERR_ADDRESS) abort();
        g_checked++;
      }
    }
    fdgpu_precompile_info_t info;
    code = fdt_secp256k1_verdict_core(
        w.code, w.instr_idx, w.rec_idx, w.ed_instr_cnt, w.rec_cnt, [&](uint32_t k) { return (int)codes[k]; },
        [&](uint32_t k) { return ((uint32_t)recs[k].instr_idx << 16) | recs[k].rec_idx; }, &info);
    if (info.sig_cnt != w.rec_cnt || info.ed_instr_cnt != w.ed_instr_cnt) abort();
    *rec_cnt = w.rec_cnt;
    *rec_code = info.ed_code;
    free(codes); free(recs); free(t);
  }
  free(p);
  return code;
}

static int vectors(const char *path, unsigned long *n_hash, unsigned long *n_rec) {
  FILE *f = fopen(path, "rb");
  if (!f) { perror(path); return 2; }
  for (;;) {
    uint8_t kind;
    if (fread(&kind, 1, 1, f) != 1) break;
    if (kind == 1) {
      uint8_t b[4], want[32], got[32];
      if (fread(b, 1, 4, f) != 4) return 2;
      const uint32_t sz = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
      uint8_t *m = (uint8_t *)malloc(sz ? sz : 1);             /* exact size */
      if (!m || (sz && fread(m, 1, sz, f) != sz) || fread(want, 1, 32, f) != 32) return 2;
      fdt_keccak256_core(m, sz, got);
      free(m);
      if (memcmp(got, want, 32)) { fprintf(stderr, "keccak vector %lu (%u bytes) differs\n", *n_hash, sz); return 1; }
      ++*n_hash;
    } else if (kind == 2) {
      uint8_t *in = (uint8_t *)malloc(97), want[65];
      if (!in || fread(in, 1, 97, f) != 97 || fread(want, 1, 65, f) != 65) return 2;
      fdt_keccak_plain_reader r{in};
      fdt_u256 h, sr, ss, x, y;
      fdt_u256_load_be(h, r, 0);
      fdt_u256_load_be(sr, r, 32);
      fdt_u256_load_be(ss, r, 64);
      const int rc = fdt_secp256k1_recover_core(h, sr, ss, in[96], x, y);
      uint8_t key[64];
      for (int i = 0; i < 8; i++)
        for (int k = 0; k < 4; k++) {
          key[4 * (7 - i) + k] = (uint8_t)(x.v[i] >> (8 * (3 - k)));
          key[32 + 4 * (7 - i) + k] = (uint8_t)(y.v[i] >> (8 * (3 - k)));
        }
      free(in);
      if (rc != (int8_t)want[0] || memcmp(key, want + 1, 64)) {
        fprintf(stderr, "recover vector %lu: code %d, expected %d (or the key differs)\n", *n_rec, rc, (int8_t)want[0]);
        return 1;
      }
      ++*n_rec;
    } else {
      fprintf(stderr, "bad vector kind %u\n", kind);
      return 2;
    }
  }
  fclose(f);
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 5) { fprintf(stderr, "usage: %s cases.bin vectors.bin random_cnt record_cnt\n", argv[0]); return 2; }
  const unsigned long random_cnt = strtoul(argv[3], nullptr, 0);
  g_budget = strtoul(argv[4], nullptr, 0);
  unsigned long n_hash = 0, n_rec = 0;
  if (const int rc = vectors(argv[2], &n_hash, &n_rec)) return rc;
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::mt19937_64 rng(0x5eed);
  std::vector<std::vector<uint8_t>> tmpl;
  unsigned long cases = 0;
  for (;;) {
    uint8_t hdr[9];
    if (fread(hdr, 1, 9, f) != 9) break;
    const uint32_t sz = (uint32_t)hdr[0] | ((uint32_t)hdr[1] << 8) | ((uint32_t)hdr[2] << 16) | ((uint32_t)hdr[3] << 24);
    const uint32_t flags = hdr[4];
    const int want = (int8_t)hdr[5], want_rc = (int8_t)hdr[6];
    const uint32_t want_cnt = (uint32_t)hdr[7] | ((uint32_t)hdr[8] << 8);
    std::vector<uint8_t> v(sz);
    if (sz && fread(v.data(), 1, sz, f) != sz) { fprintf(stderr, "short case file\n"); return 2; }
    uint32_t cnt = 0;
    int rc = 0;
    const int got = run(v, flags, true, &cnt, &rc);
    if (got != want || cnt != want_cnt || rc != want_rc) {
      fprintf(stderr, "case %lu: got %d (record code %d) with %u records, expected %d (%d) with %u\n", cases, got, rc, cnt,
              want, want_rc, want_cnt);
      return 1;
    }
    if (got != FDGPU_CODE_PARSE_FAIL && !flags) tmpl.push_back(v);
    cases++;
  }
  fclose(f);
  if (tmpl.empty()) { fprintf(stderr, "no parsing case to mutate\n"); return 2; }
  g_checked = 0;
  unsigned long parsed = 0, recs = 0;
  for (unsigned long k = 0; k < random_cnt; k++) {
    std::vector<uint8_t> v = tmpl[rng() % tmpl.size()];
    const int nm = 1 + (int)(rng() % 3);
    for (int j = 0; j < nm && !v.empty(); j++) {
      /* past the 166 bytes of signature, header, accounts and blockhash lie the instructions */
      const size_t at = v.size() > 170 && rng() % 4 ? 165 + rng() % (v.size() - 165) : rng() % v.size();
      v[at] = rng() % 2 ? (uint8_t)(v[at] ^ (1u << (rng() & 7))) : (uint8_t)rng();
    }
    if (rng() % 16 == 0) v.resize(rng() % (v.size() + 1));
    uint32_t cnt = 0;
    int rc = 0;
    parsed += run(v, (uint32_t)(k & 1), false, &cnt, &rc) != FDGPU_CODE_PARSE_FAIL;
    recs += cnt;
  }
  printf("vectors %lu keccak, %lu recover ok; cases %lu ok, random %lu: %lu parsed, %lu records, %lu checked\n", n_hash,
         n_rec, cases, random_cnt, parsed, recs, g_checked);
  return 0;
}
