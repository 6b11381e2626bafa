/* precompile_san.cpp -- fdt_precompile_walk_core / fdt_precompile_verdict_core (firedancer_amd/csrc/fdt_precompile.h, the
   source both the host library and the GPU kernel compile) behind fdt_parse_core, under the sanitizers, as a program
   of its own:

     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include \
         tools/precompile_san.cpp -o precompile_san
     ./precompile_san cases.bin <random_cnt>

   cases.bin: records [u32 size][i8 expected structural code: 0, -70, -71, or -64 when the payload does not parse]
   [u16 expected record count][size bytes].  Then random_cnt buffers: mutations (one to three bytes, biased towards
   the instruction data; now and then a truncation) of the cases that parse.  Every payload, every parsed fd_txn_t and
   every record array lives in a heap allocation of exactly its size, so a read or write past it is an error the
   sanitizer reports.  The verdict runs over codes that fail at a random record.  tests/test_precompile.py builds and
   runs it. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../firedancer_amd/csrc/fdt_precompile.h"

struct store {
  fdt_precompile_rec_t *recs;
  uint32_t cap, n;
  void operator()(uint32_t j, uint32_t i, uint32_t s, uint32_t p, uint32_t m, uint32_t ms) {
    if (n < cap) recs[n] = {(uint16_t)j, (uint16_t)i, (uint16_t)s, (uint16_t)p, (uint16_t)m, (uint16_t)ms};
    n++;
  }
};
struct count {
  void operator()(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {}
};

/* -> the structural code (or -64), *rec_cnt the records emitted */
static int run(const std::vector<uint8_t> &v, uint32_t *rec_cnt, std::mt19937_64 &rng) {
  uint8_t *p = (uint8_t *)malloc(v.size() ? v.size() : 1);    /* exact size: no slack behind the payload */
  if (!p) abort();
  if (!v.empty()) memcpy(p, v.data(), v.size());
  uint64_t fail = 0;
  *rec_cnt = 0;
  const uint64_t fp = fdt_parse_core(p, v.size(), nullptr, &fail);
  int code = FDGPU_CODE_PARSE_FAIL;
  if (fp) {
    if (fp > FDT_TXN_MAX_SZ) abort();
    fdt_txn_t *t = (fdt_txn_t *)malloc(fp);                    /* exact size: the footprint the parser reported */
    if (!t || fdt_parse_core(p, v.size(), t, &fail) != fp) abort();
    fdt_precompile_walk_t w, w2;
    count c;
    fdt_precompile_walk_core(p, v.size(), t, c, &w);
    if (w.rec_cnt > fdt_precompile_sig_bound(v.size())) abort();
    fdt_precompile_rec_t *recs = (fdt_precompile_rec_t *)malloc(w.rec_cnt ? w.rec_cnt * sizeof *recs : 1);
    int8_t *codes = (int8_t *)calloc(w.rec_cnt ? w.rec_cnt : 1, 1);
    if (!recs || !codes) abort();
    store st{recs, w.rec_cnt, 0};
    fdt_precompile_walk_core(p, v.size(), t, st, &w2);
    if (st.n != w.rec_cnt || w2.rec_cnt != w.rec_cnt || w2.code != w.code || w2.instr_idx != w.instr_idx ||
        w2.rec_idx != w.rec_idx || w2.ed_instr_cnt != w.ed_instr_cnt)
      abort();
    for (uint32_t k = 0; k < w.rec_cnt; k++) {
      const fdt_precompile_rec_t &q = recs[k];
      if ((uint64_t)q.sig_off + 64 > v.size() || (uint64_t)q.pub_off + 32 > v.size() ||
          (uint64_t)q.msg_off + q.msg_sz > v.size() || q.instr_idx >= t->instr_cnt)
        abort();
      volatile uint8_t sink = p[q.sig_off + 63] ^ p[q.pub_off + 31] ^ (q.msg_sz ? p[q.msg_off + q.msg_sz - 1] : 0);
      (void)sink;
    }
    const uint32_t bad = w.rec_cnt ? (uint32_t)(rng() % (2 * w.rec_cnt)) : 0;   /* half the time: none fails */
    if (bad < w.rec_cnt) codes[bad] = (int8_t)-(1 + (int)(rng() % 3));
    fdgpu_precompile_info_t info;
    const int vd = fdt_precompile_verdict_core(
        w.code, w.instr_idx, w.rec_idx, w.ed_instr_cnt, w.rec_cnt, [&](uint32_t k) { return (int)codes[k]; },
        [&](uint32_t k) { return ((uint32_t)recs[k].instr_idx << 16) | recs[k].rec_idx; }, &info);
    if (bad < w.rec_cnt ? (vd != FDGPU_CODE_PRECOMPILE_SIGNATURE || info.instr_idx != recs[bad].instr_idx ||
                           info.rec_idx != recs[bad].rec_idx || info.ed_code != codes[bad])
                        : (vd != w.code || info.ed_code != 0 || info.instr_idx != w.instr_idx))
      abort();
    if (info.sig_cnt != w.rec_cnt || info.ed_instr_cnt != w.ed_instr_cnt) abort();
    code = w.code;
    *rec_cnt = w.rec_cnt;
    free(codes); free(recs); free(t);
  }
  free(p);
  return code;
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s cases.bin random_cnt\n", argv[0]); return 2; }
  const unsigned long random_cnt = strtoul(argv[2], nullptr, 0);
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::mt19937_64 rng(0x5eed);
  std::vector<std::vector<uint8_t>> tmpl;
  unsigned long cases = 0;
  for (;;) {
    uint8_t hdr[7];
    if (fread(hdr, 1, 7, f) != 7) break;
    const uint32_t sz = (uint32_t)hdr[0] | ((uint32_t)hdr[1] << 8) | ((uint32_t)hdr[2] << 16) | ((uint32_t)hdr[3] << 24);
    const int want = (int8_t)hdr[4];
    const uint32_t want_cnt = (uint32_t)hdr[5] | ((uint32_t)hdr[6] << 8);
    std::vector<uint8_t> v(sz);
    if (sz && fread(v.data(), 1, sz, f) != sz) { fprintf(stderr, "short case file\n"); return 2; }
    uint32_t cnt = 0;
    const int got = run(v, &cnt, rng);
    if (got != want || cnt != want_cnt) {
      fprintf(stderr, "case %lu: got %d with %u records, expected %d with %u\n", cases, got, cnt, want, want_cnt);
      return 1;
    }
    if (got != FDGPU_CODE_PARSE_FAIL) tmpl.push_back(v);
    cases++;
  }
  fclose(f);
  if (tmpl.empty()) { fprintf(stderr, "no parsing case to mutate\n"); return 2; }
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
    parsed += run(v, &cnt, rng) != FDGPU_CODE_PARSE_FAIL;
    recs += cnt;
  }
  printf("cases %lu ok, random %lu: %lu parsed, %lu records\n", cases, random_cnt, parsed, recs);
  return 0;
}
