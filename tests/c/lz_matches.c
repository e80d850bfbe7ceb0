/* lz_matches.c -- the LZMA coder's match finder and the parser on supplied lists under AddressSanitizer / UndefinedBehaviorSanitizer: a
 * stand-alone program (its own main, never loaded into Python, never run on a GPU machine).  For every input -- each length 0 .. 40 over
 * four symbols, runs, "ab" repeated past the parse window, records with one changing field, and the stream named on the command line
 * (tests/golden/football_cif_kf1.lzma, decoded) -- held in an allocation of its exact size:
 *   tm_lz_matches_host of the whole stream into arrays of exactly the sizes it reported, and again in windows: the same lists;
 *   tm_lz_compress_from_matches_host on those lists: tm_lz_compress_host's bytes.
 * Build and run: tools/asan_lz_matches.sh (this file with clang -fsanitize=address,undefined; tm_lzma.hip and tm_tables.hip with hipcc
 * -Xarch_host -fsanitize=address,undefined; no device is touched). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tilemotion.h"

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((lcg_state >> 33) % n);
}

static void fail(const char *what, size_t n) {
  fprintf(stderr, "%s (stream of %zu bytes): %s\n", what, n, tm_last_error() ? tm_last_error() : "");
  exit(2);
}

static long streams = 0, pairs_seen = 0;

static void check_stream(const uint8_t *data, size_t n) {
  uint8_t *src = (uint8_t *)malloc(n ? n : 1);
  if (n) memcpy(src, data, n);
  uint8_t *counts = (uint8_t *)malloc(n ? n : 1);
  size_t need = 0;
  int rc = tm_lz_matches_host(n ? src : NULL, n, 0, n, counts, NULL, 0, &need);
  if (rc != TM_OK && !(rc == TM_E_INVAL && need > 0)) fail("matches: size query", n);
  tm_lz_pair *pairs = (tm_lz_pair *)malloc(need ? need * sizeof(tm_lz_pair) : 1);
  size_t got = 0;
  if (tm_lz_matches_host(n ? src : NULL, n, 0, n, counts, pairs, need, &got) != TM_OK || got != need) fail("matches", n);
  /* in windows of 1000 positions, each into arrays of its exact size */
  size_t at = 0;
  for (size_t first = 0; first < n; first += 1000) {
    const size_t count = n - first < 1000 ? n - first : 1000;
    uint8_t *wc = (uint8_t *)malloc(count);
    size_t wn = 0;
    for (size_t i = 0; i < count; i++) wn += counts[first + i];
    tm_lz_pair *wp = (tm_lz_pair *)malloc(wn ? wn * sizeof(tm_lz_pair) : 1);
    size_t wgot = 0;
    if (tm_lz_matches_host(src, n, first, count, wc, wp, wn, &wgot) != TM_OK || wgot != wn) fail("matches of a window", n);
    if (memcmp(wc, counts + first, count) || (wn && memcmp(wp, pairs + at, wn * sizeof(tm_lz_pair)))) fail("a window's lists differ from the whole stream's", n);
    at += wn;
    free(wc); free(wp);
  }
  size_t want_n = 0, out_n = 0;
  tm_lz_compress_host(n ? src : NULL, n, NULL, 0, &want_n);
  uint8_t *want = (uint8_t *)malloc(want_n), *out = (uint8_t *)malloc(want_n);
  if (tm_lz_compress_host(n ? src : NULL, n, want, want_n, &want_n) != TM_OK) fail("compress", n);
  if (tm_lz_compress_from_matches_host(n ? src : NULL, n, counts, pairs, out, want_n, &out_n) != TM_OK || out_n != want_n || memcmp(out, want, want_n))
    fail("the parser on supplied lists writes another stream", n);
  streams++;
  pairs_seen += (long)need;
  free(src); free(counts); free(pairs); free(want); free(out);
}

int main(int argc, char **argv) {
  uint8_t *buf = (uint8_t *)malloc(1 << 20);
  for (size_t n = 0; n <= 40; n++) {
    for (size_t i = 0; i < n; i++) buf[i] = (uint8_t)rnd(4);
    check_stream(buf, n);
  }
  size_t n = 0;
  for (int r = 0; r < 40; r++) { const size_t len = 1 + rnd(3000); memset(buf + n, r, len); n += len; }  /* runs of one byte */
  check_stream(buf, n);
  for (n = 0; n < 8193; n++) buf[n] = n & 1 ? 'b' : 'a';
  for (size_t i = 0; i < 50; i++) buf[n++] = (uint8_t)rnd(256);
  check_stream(buf, n);
  uint8_t rec[24];
  for (int i = 0; i < 24; i++) rec[i] = (uint8_t)rnd(256);
  for (n = 0; n < 24 * 2000; n += 24) { memcpy(buf + n, rec, 24); buf[n + 5] = (uint8_t)rnd(4); }  /* one changing field */
  check_stream(buf, n);
  free(buf);
  if (argc > 1) {
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    const size_t zn = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *z = (uint8_t *)malloc(zn);
    if (fread(z, 1, zn, f) != zn) { fprintf(stderr, "short read\n"); return 2; }
    fclose(f);
    size_t raw_n = 0;
    tm_lz_decompress_host(z, zn, NULL, 0, &raw_n, NULL);
    uint8_t *raw = (uint8_t *)malloc(raw_n ? raw_n : 1);
    if (tm_lz_decompress_host(z, zn, raw, raw_n, &raw_n, NULL) != TM_OK) fail("decompress", zn);
    check_stream(raw, raw_n);
    free(z); free(raw);
  }
  printf("lz_matches: %ld streams, %ld pairs, no finding\n", streams, pairs_seen);
  return 0;
}
