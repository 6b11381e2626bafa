/* shred_san.cpp -- fdt_shred_check_core / fdt_shred_root_core (firedancer_amd/csrc/fdt_shred.h, the source both the
   host library and the GPU kernel compile) under the sanitizers, as a program of its own:

     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include \
         tools/shred_san.cpp -o shred_san
     ./shred_san cases.bin <expected_version> <random_cnt>

   cases.bin: records [u32 size][u8 expect: 1 passes the checks, 0 dropped][size bytes]; the first record that passes is
   also the template the mutated buffers start from.  Then random_cnt buffers: half random bytes of random size with a
   plausible header, half single- or double-byte mutations (and truncations) of the template.  Every buffer lives in a
   heap allocation of exactly its size, so a read past it is an error the sanitizer reports.  tests/test_shred.py builds
   and runs it. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../firedancer_amd/csrc/fdt_shred.h"

static int run(const std::vector<uint8_t> &v, uint16_t version, uint8_t root[32]) {
  uint8_t *p = (uint8_t *)malloc(v.size() ? v.size() : 1);    /* exact size: no slack behind the shred */
  if (!p) abort();
  if (!v.empty()) memcpy(p, v.data(), v.size());
  fdt_shred_chk_t chk;
  const int ok = fdt_shred_check_core(p, v.size(), version, &chk);
  if (ok) {
    if (chk.leaf_off != 64 || chk.leaf_end != chk.proof_off || chk.proof_off + 20ull * chk.depth > v.size()) abort();
    fdt_shred_root_core(p, &chk, root);
  }
  free(p);
  return ok;
}

int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s cases.bin version random_cnt\n", argv[0]); return 2; }
  const uint16_t version = (uint16_t)strtoul(argv[2], nullptr, 0);
  const unsigned long random_cnt = strtoul(argv[3], nullptr, 0);
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint8_t> tmpl;
  unsigned long cases = 0;
  uint8_t root[32];
  for (;;) {
    uint8_t hdr[5];
    if (fread(hdr, 1, 5, f) != 5) break;
    const uint32_t sz = (uint32_t)hdr[0] | ((uint32_t)hdr[1] << 8) | ((uint32_t)hdr[2] << 16) | ((uint32_t)hdr[3] << 24);
    std::vector<uint8_t> v(sz);
    if (sz && fread(v.data(), 1, sz, f) != sz) { fprintf(stderr, "short case file\n"); return 2; }
    const int ok = run(v, version, root);
    if (ok != hdr[4]) { fprintf(stderr, "case %lu: got %d, expected %d\n", cases, ok, (int)hdr[4]); return 1; }
    if (ok && tmpl.empty()) tmpl = v;
    cases++;
  }
  fclose(f);
  if (tmpl.empty()) { fprintf(stderr, "no passing case to mutate\n"); return 2; }
  std::mt19937_64 rng(0x5eed);
  unsigned long passed = 0;
  static const uint8_t variants[] = {0x80, 0x40, 0x90, 0x60, 0xb0, 0x70, 0xa5, 0x5a, 0x30};
  for (unsigned long k = 0; k < random_cnt; k++) {
    std::vector<uint8_t> v;
    if (k & 1) {
      v = tmpl;
      const int nm = 1 + (int)(rng() & 1);
      for (int j = 0; j < nm; j++) v[(rng() % 4 ? rng() % 0x5a : rng() % v.size())] ^= (uint8_t)(1u << (rng() & 7));
      if (rng() % 8 == 0) v.resize(rng() % (v.size() + 1));
    } else {
      static const size_t sizes[] = {0, 1, 87, 88, 89, 1202, 1203, 1204, 1227, 1228, 1229, 1232};
      v.resize(rng() % 4 ? sizes[rng() % 12] : rng() % 1300);
      for (auto &b : v) b = (uint8_t)rng();
      if (v.size() > 0x58 && rng() % 2) {
        v[0x40] = (uint8_t)(variants[rng() % 9] | (rng() & 0xf));
        v[0x4d] = (uint8_t)version; v[0x4e] = (uint8_t)(version >> 8);
        if (rng() % 2) { v[0x53] = (uint8_t)(rng() % 70); v[0x54] = 0; v[0x55] = (uint8_t)(rng() % 70); v[0x56] = 0; v[0x57] = (uint8_t)(rng() % 70); v[0x58] = 0; }
        else { memcpy(&v[0x4f], &v[0x49], 4); v[0x49] = (uint8_t)(v[0x49] + rng() % 70); v[0x56] = (uint8_t)rng(); v[0x57] = (uint8_t)(rng() % 5); }
      }
    }
    passed += (unsigned long)run(v, version, root);
  }
  printf("cases %lu ok, random %lu: %lu passed the checks\n", cases, random_cnt, passed);
  return 0;
}
