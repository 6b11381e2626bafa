/* shred_sets_san.cpp -- the host rule of a set batch (firedancer_amd/csrc/fdt_shred_sets.h, the source
   fdgpu_shred_sets_verify compiles: argument check, states, grouping by key, scatter) with the roots of
   firedancer_amd/csrc/fdt_shred.h, under the sanitizers, as a program of its own:

     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include \
         tools/shred_sets_san.cpp -o shred_sets_san
     ./shred_sets_san batch.bin <expected_version> <random_cnt>

   batch.bin: [u32 n][u32 arena_sz][arena][n records of 16 B][n expected codes, i8][n expected representatives, u32]
   [u32 expected lanes], the codes with every verify answering 0.  Then random_cnt batches drawn from it: a random
   choice of its records, now and then with an offset or a known root moved to the arena's last bytes or past them.
   Every arena lives in a heap allocation of exactly its size and the outputs in allocations of exactly n items, so a
   read or write past them is an error the sanitizer reports.  tests/test_shredsets.py builds and runs it. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../firedancer_amd/csrc/fdt_shred.h"
#include "../firedancer_amd/csrc/fdt_shred_sets.h"

struct Out {
  std::vector<int8_t> codes;
  std::vector<uint32_t> rep;
  uint32_t lanes = 0;
};

/* -1: the arguments were refused; else 0 and the batch's outputs (every verify answers 0) */
static int run(const std::vector<uint8_t> &arena_v, const std::vector<fdgpu_set_shred_t> &recs_v, uint16_t version, Out &o) {
  const uint64_t n = recs_v.size(), arena_sz = arena_v.size();
  uint8_t *arena = (uint8_t *)malloc(arena_sz ? arena_sz : 1);          /* exact sizes: no slack behind anything */
  fdgpu_set_shred_t *recs = (fdgpu_set_shred_t *)malloc(n ? n * sizeof(fdgpu_set_shred_t) : 1);
  uint8_t *roots = (uint8_t *)malloc(n ? 32 * n : 1), *ok = (uint8_t *)malloc(n ? n : 1);
  int8_t *codes = (int8_t *)malloc(n ? n : 1);
  uint32_t *rep = (uint32_t *)malloc(n ? 4 * n : 1);
  if (!arena || !recs || !roots || !ok || !codes || !rep) abort();
  if (arena_sz) memcpy(arena, arena_v.data(), arena_sz);
  if (n) memcpy(recs, recs_v.data(), n * sizeof(fdgpu_set_shred_t));
  int rc = -1;
  if (fdt_shred_sets_args(arena_sz, recs, n)) {
    for (uint64_t i = 0; i < n; i++) {
      fdt_shred_chk_t chk;
      ok[i] = (uint8_t)fdt_shred_check_core(arena + recs[i].off, recs[i].sz, version, &chk);
      if (ok[i]) fdt_shred_root_core(arena + recs[i].off, &chk, roots + 32 * i);
      else memset(roots + 32 * i, 0, 32);
    }
    std::vector<uint32_t> reps;
    fdt_shred_sets_group(arena, recs, n, ok, roots, codes, rep, reps);
    std::vector<int8_t> rep_codes(reps.size() ? reps.size() : 1, 0);
    fdt_shred_sets_scatter(n, rep, reps, rep_codes.data(), codes);
    /* what holds of any batch */
    for (uint64_t i = 0; i < n; i++) {
      const uint32_t r = rep[i];
      const bool cand = ok[i] && recs[i].known_off == FDGPU_SHRED_NO_ROOT;
      if (cand != (r != UINT32_MAX)) abort();
      if (!cand) continue;
      if (r > i || rep[r] != r) abort();
      if (memcmp(arena + recs[i].off, arena + recs[r].off, 64) || memcmp(roots + 32 * i, roots + 32 * r, 32) ||
          memcmp(arena + recs[i].pub_off, arena + recs[r].pub_off, 32))
        abort();
    }
    o.codes.assign(codes, codes + n);
    o.rep.assign(rep, rep + n);
    o.lanes = (uint32_t)reps.size();
    rc = 0;
  }
  free(arena); free(recs); free(roots); free(ok); free(codes); free(rep);
  return rc;
}

static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s batch.bin version random_cnt\n", argv[0]); return 2; }
  const uint16_t version = (uint16_t)strtoul(argv[2], nullptr, 0);
  const unsigned long random_cnt = strtoul(argv[3], nullptr, 0);
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<uint8_t> file;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + k);
  fclose(f);
  if (file.size() < 8) { fprintf(stderr, "short batch file\n"); return 2; }
  const uint64_t n = rd32(&file[0]), arena_sz = rd32(&file[4]);
  if (file.size() != 8 + arena_sz + 16 * n + n + 4 * n + 4) { fprintf(stderr, "batch file size\n"); return 2; }
  const std::vector<uint8_t> arena(file.begin() + 8, file.begin() + 8 + arena_sz);
  const uint8_t *q = &file[8 + arena_sz];
  std::vector<fdgpu_set_shred_t> recs(n);
  for (uint64_t i = 0; i < n; i++, q += 16) recs[i] = {rd32(q), rd32(q + 4), rd32(q + 8), rd32(q + 12)};
  const int8_t *want_codes = (const int8_t *)q;
  const uint8_t *want_rep = q + n, *want_lanes = q + 5 * n;
  Out o;
  if (run(arena, recs, version, o)) { fprintf(stderr, "the batch's arguments were refused\n"); return 1; }
  for (uint64_t i = 0; i < n; i++)
    if (o.codes[i] != want_codes[i] || o.rep[i] != rd32(want_rep + 4 * i)) {
      fprintf(stderr, "shred %llu: code %d rep %u, expected %d %u\n", (unsigned long long)i, o.codes[i], o.rep[i],
              want_codes[i], rd32(want_rep + 4 * i));
      return 1;
    }
  if (o.lanes != rd32(want_lanes)) { fprintf(stderr, "lanes %u, expected %u\n", o.lanes, rd32(want_lanes)); return 1; }
  std::mt19937_64 rng(0x5e75);
  unsigned long ran = 0, refused = 0;
  for (unsigned long k = 0; k < random_cnt && n; k++) {
    std::vector<fdgpu_set_shred_t> r(rng() % 97);
    bool bad = false;
    for (auto &x : r) {
      x = recs[rng() % n];
      switch (rng() % 16) {
        case 0: x.known_off = (uint32_t)arena_sz - 32; break;                 /* the arena's last 32 bytes */
        case 1: x.known_off = (uint32_t)arena_sz - 31; bad = true; break;     /* one past them */
        case 2: x.pub_off = (uint32_t)arena_sz - 32; break;
        case 3: x.pub_off = (uint32_t)arena_sz - (uint32_t)(rng() % 32); bad = true; break;
        case 4: x.off = (uint32_t)arena_sz - x.sz; break;
        case 5: x.off = (uint32_t)arena_sz - x.sz + 1 + (uint32_t)(rng() % 64); bad = true; break;
        case 6: x.sz = (uint32_t)(rng() % (x.sz + 1)); break;                 /* truncated: the checks decide */
        case 7: x.known_off = x.off + (uint32_t)(rng() % 64); break;          /* some 32 bytes: a mismatch */
        default: break;
      }
    }
    Out o2;
    const int rc = run(arena, r, version, o2);
    if ((rc != 0) != bad) { fprintf(stderr, "random batch %lu: refused %d, expected %d\n", k, rc != 0, (int)bad); return 1; }
    if (rc) refused++; else ran++;
  }
  printf("batch %llu ok, lanes %u, random %lu: %lu ran, %lu refused\n", (unsigned long long)n, o.lanes, random_cnt, ran, refused);
  return 0;
}
