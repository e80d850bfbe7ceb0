/* png_inflate.c -- the PNG reader's rule (tm_inflate.h, through its host twins in tm_png_in.hip) under AddressSanitizer /
 * UndefinedBehaviorSanitizer: a stand-alone program (its own main, never loaded into Python, never run on a GPU machine).  The kernels
 * compile the same text, so what is out of bounds here would be out of bounds there.  Every source and every destination sits in an
 * allocation of its exact size:
 *   the cases of tests/png_in_cases.py (`python tests/png_in_cases.py FILE` writes them): streams that decode, the damaged list, pictures
 *   that decode, damaged pictures -- tm_inflate_streams_host against tm_inflate_host, tm_png_decode_host against tm_read_png_host: the
 *   same verdict, and the same bytes when accepted;
 *   a seeded fuzz of the rule: every stream that decodes with 1-3 bytes overwritten, cut short, or replaced by noise behind its header,
 *   its input cut into random spans (empty ones among them), its destination exact, one byte short or larger; every small picture with
 *   bytes of its IDAT payload overwritten and the chunk's CRC mended.
 * Build and run: tools/asan_png_in.sh (this file with clang -fsanitize=address,undefined; tm_png_in.hip, tm_png.hip and tm_tables.hip with
 * hipcc -Xarch_host -fsanitize=address,undefined; no device is touched). */
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

static void fail(const char *what, long n) {
  fprintf(stderr, "%s (%ld): %s\n", what, n, tm_last_error() ? tm_last_error() : "");
  exit(2);
}

static long n_streams = 0, n_accepted = 0, n_pictures = 0, n_pictures_ok = 0;

static void *exact(size_t n) {  /* an allocation of n bytes (of 1 when n is 0: never read or written then) */
  void *p = malloc(n ? n : 1);
  if (!p) fail("out of memory", (long)n);
  return p;
}

/* z: the joined stream.  Decoded through `nspans` spans cut at `cuts` (ascending, within [0, n]) and through the old reader: the same
 * verdict and bytes.  want: the data when the stream is known to decode (else NULL).  Returns 1 when accepted. */
static int check_stream(const uint8_t *z, size_t n, const uint32_t *cuts, int nspans, uint32_t cap, const uint8_t *want, size_t want_n, int must_refuse) {
  uint8_t *blob = (uint8_t *)exact(n);
  if (n) memcpy(blob, z, n);
  tm_inflate_span *spans = (tm_inflate_span *)exact((size_t)nspans * sizeof(tm_inflate_span));
  for (int j = 0; j < nspans; j++) {
    const uint32_t from = j ? cuts[j - 1] : 0, to = j + 1 < nspans ? cuts[j] : (uint32_t)n;
    spans[j].off = from; spans[j].len = to - from; spans[j].reserved = 0;
  }
  tm_inflate_stream st = {0, cap, 0, (uint32_t)nspans, 0};
  tm_inflate_status status = {-1, 0, 0};
  uint8_t *dst = (uint8_t *)exact(cap), *old = (uint8_t *)exact(cap);
  if (tm_inflate_streams_host(blob, n, spans, nspans, &st, 1, dst, cap, &status) != TM_OK) fail("tm_inflate_streams_host refused the batch", (long)n);
  size_t old_n = 0;
  const int old_rc = tm_inflate_host(blob, n, old, cap, &old_n);
  if ((old_rc == TM_OK) != (status.code == 0)) fail("the two readers disagree about a stream", status.code);
  if (status.in_pos > n) fail("an input position past the stream", (long)status.in_pos);
  if (old_rc == TM_OK) {
    if (status.out_n != old_n || (old_n && memcmp(dst, old, old_n))) fail("the two readers' bytes differ", (long)old_n);
    if (want && (old_n != want_n || (want_n && memcmp(dst, want, want_n)))) fail("not the data", (long)want_n);
  } else if (want && cap >= want_n) fail("a stream that decodes was refused", status.code);
  if (must_refuse && status.code == 0) fail("a damaged stream was accepted", (long)n);
  free(blob); free(spans); free(dst); free(old);
  n_streams++;
  n_accepted += status.code == 0;
  return status.code == 0;
}

static void fuzz_stream(const uint8_t *z, size_t n, size_t data_n) {
  if (n < 3) return;
  const int rounds = n < 8192 ? 300 : n < 100000 ? 40 : 6;
  uint8_t *bad = (uint8_t *)exact(n + 200);
  for (int r = 0; r < rounds; r++) {
    size_t bn = n;
    memcpy(bad, z, n);
    const uint32_t kind = rnd(4);
    if (kind < 2) {
      for (uint32_t k = 1 + rnd(3); k > 0; k--) bad[rnd((uint32_t)n)] = (uint8_t)rnd(256);
    } else if (kind == 2) {
      bn = rnd((uint32_t)n);
    } else {
      bn = 2 + rnd(200);
      for (size_t k = 2; k < bn; k++) bad[k] = (uint8_t)rnd(256);
    }
    uint32_t cuts[6];
    const int nspans = 1 + (int)rnd(6);
    for (int j = 0; j + 1 < nspans; j++) cuts[j] = rnd((uint32_t)bn + 1);
    for (int a = 0; a + 1 < nspans; a++)
      for (int b = a + 1; b + 1 < nspans; b++)
        if (cuts[b] < cuts[a]) { const uint32_t t = cuts[a]; cuts[a] = cuts[b]; cuts[b] = t; }
    const uint32_t pick = rnd(4);
    const uint32_t cap = pick == 0 && data_n ? (uint32_t)data_n - 1 : pick == 1 ? (uint32_t)data_n + 1 + rnd(300) : (uint32_t)data_n;
    check_stream(bad, bn, cuts, nspans, cap, NULL, 0, 0);
  }
  free(bad);
}

static uint32_t crc_table[256];
static uint32_t crc32_of(const uint8_t *p, size_t n) {
  if (!crc_table[1])
    for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1; crc_table[i] = c; }
  uint32_t crc = 0xffffffffu;
  for (size_t i = 0; i < n; i++) crc = crc_table[(crc ^ p[i]) & 0xff] ^ (crc >> 8);
  return ~crc;
}

/* one file through both readers: the same verdict, the same pixels.  Returns 1 when it decodes. */
static int check_picture(const uint8_t *png, size_t n, int w, int h, const char *tmp, int must_decode, int must_refuse) {
  uint8_t *file = (uint8_t *)exact(n);
  memcpy(file, png, n);
  const size_t px = (size_t)w * h;
  uint32_t *out = (uint32_t *)exact(px * 4), *old = (uint32_t *)exact(px * 4);
  const void *files[1] = {file};
  const size_t sizes[1] = {n};
  int32_t status = -1;
  const int rc = tm_png_decode_host(files, sizes, 1, w, h, out, (int64_t)px, &status);
  FILE *f = fopen(tmp, "wb");
  if (!f || fwrite(file, 1, n, f) != n) fail("cannot write the temporary file", (long)n);
  fclose(f);
  int ow = 0, oh = 0;
  const int old_rc = tm_read_png_host(tmp, old, (int64_t)px, &ow, &oh);
  const int ok = rc == TM_OK && status == 0;
  if (ok != (old_rc == TM_OK)) fail("the two readers disagree about a picture", status);
  if (ok && (ow != w || oh != h || memcmp(out, old, px * 4))) fail("the two readers' pixels differ", (long)px);
  if (must_decode && !ok) fail("a picture that decodes was refused", status);
  if (must_refuse && (ok || rc != TM_OK)) fail("a damaged picture: accepted, or refused by the container walk", rc);
  free(file); free(out); free(old);
  n_pictures++;
  n_pictures_ok += ok;
  return ok;
}

static void fuzz_picture(const uint8_t *png, size_t n, int w, int h, const char *tmp) {
  /* the first IDAT chunk with a payload */
  size_t at = 8;
  while (at + 12 <= n) {
    const size_t len = (size_t)png[at] << 24 | (size_t)png[at + 1] << 16 | (size_t)png[at + 2] << 8 | png[at + 3];
    if (!memcmp(png + at + 4, "IDAT", 4) && len > 0) break;
    at += 12 + len;
  }
  if (at + 12 > n) return;
  const size_t len = (size_t)png[at] << 24 | (size_t)png[at + 1] << 16 | (size_t)png[at + 2] << 8 | png[at + 3];
  uint8_t *bad = (uint8_t *)exact(n);
  for (int r = 0; r < 24; r++) {
    memcpy(bad, png, n);
    for (uint32_t k = 1 + rnd(3); k > 0; k--) bad[at + 8 + rnd((uint32_t)len)] = (uint8_t)rnd(256);
    const uint32_t crc = crc32_of(bad + at + 4, len + 4);
    bad[at + 8 + len] = (uint8_t)(crc >> 24); bad[at + 9 + len] = (uint8_t)(crc >> 16); bad[at + 10 + len] = (uint8_t)(crc >> 8); bad[at + 11 + len] = (uint8_t)crc;
    check_picture(bad, n, w, h, tmp, 0, 0);
  }
  free(bad);
}

static uint32_t get32(FILE *f) {
  uint8_t b[4];
  if (fread(b, 1, 4, f) != 4) fail("the case file is cut short", 0);
  return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}
static uint8_t *get_bytes(FILE *f, size_t n) {
  uint8_t *p = (uint8_t *)exact(n);
  if (n && fread(p, 1, n, f) != n) fail("the case file is cut short", (long)n);
  return p;
}

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: png_inflate CASES TMP_FILE\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  long cases = 0;
  for (;;) {
    uint8_t kb[4];
    if (fread(kb, 1, 4, f) != 4) break;
    const uint32_t kind = kb[0];
    cases++;
    if (kind <= 1) {
      const uint32_t cap = get32(f), nspans = get32(f);
      uint8_t *z = NULL;
      size_t n = 0;
      uint32_t *cuts = (uint32_t *)exact((size_t)nspans * 4);
      for (uint32_t j = 0; j < nspans; j++) {
        const uint32_t len = get32(f);
        uint8_t *part = get_bytes(f, len);
        z = (uint8_t *)realloc(z, n + len + 1);
        memcpy(z + n, part, len);
        free(part);
        n += len;
        cuts[j] = (uint32_t)n;
      }
      const uint32_t data_n = get32(f);
      uint8_t *data = get_bytes(f, data_n);
      if (kind == 0) {
        if (!check_stream(z, n, cuts, (int)nspans, cap, data, data_n, 0)) fail("a stream that decodes was refused", cases);
        fuzz_stream(z, n, data_n);
      } else {
        check_stream(z, n, cuts, (int)nspans, cap, NULL, 0, 1);
      }
      free(z); free(cuts); free(data);
    } else {
      const uint32_t w = get32(f), h = get32(f), n = get32(f);
      uint8_t *png = get_bytes(f, n);
      check_picture(png, n, (int)w, (int)h, argv[2], kind == 2, kind == 3);
      if (kind == 2 && (size_t)w * h <= 40000) fuzz_picture(png, n, (int)w, (int)h, argv[2]);
      free(png);
    }
  }
  fclose(f);
  remove(argv[2]);
  if (cases < 300 || n_accepted == 0 || n_accepted == n_streams || n_pictures_ok == 0 || n_pictures_ok == n_pictures) fail("the cases or the fuzz reached too little", cases);
  printf("png_inflate: %ld cases; %ld streams (%ld accepted), %ld pictures (%ld decoded): ok\n", cases, n_streams, n_accepted, n_pictures, n_pictures_ok);
  return 0;
}
