/* jpeg_decode.c -- the JPEG reader's rule (tm_jpeg.h, through its host twin in tm_jpeg_in.hip) under AddressSanitizer /
 * UndefinedBehaviorSanitizer: a stand-alone program (its own main, never loaded into Python, never run on a GPU machine).  The kernel
 * compiles the same text, so what is out of bounds here would be out of bounds there.  Every file and every plane sits in an allocation
 * of its exact size (planes at the file's own size, rows as long as the plane is wide):
 *   the cases of tests/jpeg_cases.py (`python tests/jpeg_cases.py FILE` writes them): files that decode, files the container walk
 *   refuses, files with a status -- each with the verdict the cases name;
 *   a seeded fuzz: every case cut short and with single bytes changed, several thousand files in all; whatever the verdict, no access
 *   outside the file or its planes, and a decode that ends.
 * Build and run: tools/asan_jpeg_in.sh (this file with clang -fsanitize=address,undefined; tm_jpeg_in.hip and what it needs with hipcc
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

static void fail(const char *what, long n) {
  fprintf(stderr, "%s (%ld): %s\n", what, n, tm_last_error() ? tm_last_error() : "");
  exit(2);
}

static long n_calls = 0, n_decoded = 0, n_walk_refused = 0, n_status = 0;

static void *exact(size_t n) {
  void *p = malloc(n ? n : 1);
  if (!p) fail("out of memory", (long)n);
  return p;
}

/* one file: the walk, then the decode into exact planes.  Returns the walk's code when it refuses, else the file's status (>= 0). */
static int run(const uint8_t *data, size_t n) {
  uint8_t *file = (uint8_t *)exact(n);
  if (n) memcpy(file, data, n);
  tm_jpeg_info info;
  n_calls++;
  int rc = tm_probe_jpeg_host(file, n, &info);
  if (rc != TM_OK) {
    if (rc != TM_E_IO && rc != TM_E_UNSUPPORTED) fail("the walk refused with another code", rc);
    n_walk_refused++;
    free(file);
    return rc;
  }
  const int w = info.width, h = info.height, three = info.components == 3;
  const int cw = three ? (w + info.h_samp - 1) / info.h_samp : 0, ch = three ? (h + info.v_samp - 1) / info.v_samp : 0;
  uint8_t *y = (uint8_t *)exact((size_t)w * h), *u = three ? (uint8_t *)exact((size_t)cw * ch) : NULL, *v = three ? (uint8_t *)exact((size_t)cw * ch) : NULL;
  const int64_t strides[6] = {w, (int64_t)w * h, cw, (int64_t)cw * ch, cw, (int64_t)cw * ch};
  const void *files[1] = {file};
  const size_t sizes[1] = {n};
  int32_t status = -1;
  rc = tm_jpeg_decode_host(files, sizes, 1, w, h, y, u, v, strides, &status);
  if (rc != TM_OK) fail("tm_jpeg_decode_host refused a file its walk accepts", rc);
  if (status < 0 || (status != 0 && (status < TM_JPG_TRUNCATED || status > TM_JPG_BAD_RESTART))) fail("an unknown status", status);
  if ((status == TM_JPG_BAD_RESTART) != (info.status == TM_JPG_BAD_RESTART)) fail("the probe and the decode disagree about the restart markers", status);
  if (status == 0) n_decoded++; else n_status++;
  free(y); free(u); free(v); free(file);
  return status;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 1; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) fail("short cases file", 0);
  long n_cases = 0, n_fuzz = 0;
  for (uint32_t c = 0; c < count; c++) {
    uint32_t kind = 0, len = 0;
    int32_t code = 0;
    if (fread(&kind, 4, 1, f) != 1 || fread(&code, 4, 1, f) != 1 || fread(&len, 4, 1, f) != 1) fail("short cases file", (long)c);
    uint8_t *data = (uint8_t *)exact(len);
    if (len && fread(data, 1, len, f) != len) fail("short cases file", (long)c);
    const int got = run(data, len);
    if (kind == 0 && got != 0) fail("a good case was refused", (long)c);
    if (kind != 0 && got != code) fail("a case did not reach its verdict", (long)c);
    n_cases++;
    /* the fuzz: cuts and byte changes; large files (the 60 KB APP1) get fewer rounds */
    const int rounds = len < 4096 ? 80 : 12;
    uint8_t *bad = (uint8_t *)exact(len);
    for (int r = 0; r < rounds && len > 2; r++) {
      memcpy(bad, data, len);
      size_t bn = len;
      const uint32_t how = rnd(4);
      if (how == 0) bn = rnd(len);
      else
        for (uint32_t k = how; k > 0; k--) bad[how == 1 ? rnd(len) : len / 2 + rnd(len - len / 2)] = (uint8_t)rnd(256);  /* (two in three fall into the back half: the scan) */
      (void)run(bad, bn);
      n_fuzz++;
    }
    free(bad); free(data);
  }
  fclose(f);
  printf("jpeg_decode: %ld cases, %ld fuzzed files; %ld calls: %ld decoded, %ld with a status, %ld refused by the walk\n", n_cases, n_fuzz, n_calls, n_decoded, n_status,
         n_walk_refused);
  return 0;
}
