/* webp_encode.c -- the WebP writer's rule (tm_webp_out.h, through its host twin in tm_webp_out.hip) under AddressSanitizer /
 * UndefinedBehaviorSanitizer: a stand-alone program (its own main, never loaded into Python, never run on a GPU machine).  The kernels
 * compile the same text (parse_segment, best_match, token_bits, the tables' layout), so what is out of bounds here would be out of bounds
 * there.  Every clip, every file and every canvas sits in an allocation of its exact size:
 *   the clips of tests/webp_out_cases.py (`python tests/webp_out_cases.py FILE` writes them with the restatement's files): the twin's file
 *   must be the restatement's byte for byte, into room of exactly that size; one byte less must be refused with the size and write
 *   nothing; tm_webp_bound_host must bound it; the canvas the twin returns must be the source;
 *   every clip once more at lz77 = 0, palette off and three segment sizes, each into exact room.
 * Build and run: tools/asan_webp_out.sh (this file with clang -fsanitize=address,undefined; tm_webp_out.hip and what it needs with hipcc
 * -Xarch_host -fsanitize=address,undefined; no device is touched). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tilemotion.h"

static void fail(const char *what, long n) {
  fprintf(stderr, "%s (%ld): %s\n", what, n, tm_last_error() ? tm_last_error() : "");
  exit(2);
}

static void *exact(size_t n) {
  void *p = malloc(n ? n : 1);
  if (!p) fail("out of memory", (long)n);
  return p;
}

static long n_files = 0, n_frames = 0, n_variants = 0;

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 1; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) fail("short cases file", 0);
  for (uint32_t c = 0; c < count; c++) {
    uint32_t shape[3];
    double fps = 0.0;
    int32_t o[6];
    if (fread(shape, 4, 3, f) != 3 || fread(&fps, 8, 1, f) != 1 || fread(o, 4, 6, f) != 6) fail("short cases file", (long)c);
    const int nf = (int)shape[0], w = (int)shape[1], h = (int)shape[2];
    const size_t px = (size_t)w * h;
    uint32_t *frames = (uint32_t *)exact(px * nf * 4);
    if (fread(frames, 4, px * nf, f) != px * nf) fail("short cases file", (long)c);
    uint32_t want_n = 0;
    if (fread(&want_n, 4, 1, f) != 1) fail("short cases file", (long)c);
    uint8_t *want = (uint8_t *)exact(want_n);
    if (fread(want, 1, want_n, f) != want_n) fail("short cases file", (long)c);
    tm_webp_options opt = {o[0], o[1], o[2], o[3], o[4], o[5]};

    int64_t bound = 0, need = -1;
    if (tm_webp_bound_host(w, h, nf, &opt, &bound) != TM_OK || bound < (int64_t)want_n) fail("the bound does not hold the file", (long)c);
    uint8_t *file = (uint8_t *)exact(want_n);
    uint32_t *canvas = (uint32_t *)exact(px * nf * 4);
    tm_webp_export_stats st;
    if (tm_webp_encode_host(frames, w, (int64_t)px, nf, w, h, fps, &opt, file, (int64_t)want_n - 1, &need, NULL, NULL) != TM_E_INVAL || need != (int64_t)want_n)
      fail("room one byte short was not refused with the size", (long)c);
    if (tm_webp_encode_host(frames, w, (int64_t)px, nf, w, h, fps, &opt, file, want_n, &need, canvas, &st) != TM_OK) fail("the twin refused a case", (long)c);
    if (need != (int64_t)want_n || memcmp(file, want, want_n)) fail("the twin's file is not the restatement's", (long)c);
    if (st.frames != nf || st.file_bytes != (int64_t)want_n || st.tokens < st.segments || st.matches > st.tokens) fail("the stats disagree", (long)c);
    for (size_t k = 0; k < px * nf; k++) if (canvas[k] != (frames[k] & 0xffffffu)) fail("the canvas is not the source", (long)c);
    n_files++; n_frames += nf;

    const int32_t variants[5][3] = {{0, 0, 0}, {1, 1, 0}, {1, 0, 1}, {1, 0, 7}, {1, 1, 1000}};  /* lz77, palette, segment_pixels */
    for (int v = 0; v < 5; v++) {
      tm_webp_options other = opt;
      other.lz77 = variants[v][0]; other.palette = variants[v][1]; other.segment_pixels = variants[v][2];
      int64_t n = -1, n2 = -1;
      if (tm_webp_encode_host(frames, w, (int64_t)px, nf, w, h, fps, &other, NULL, 0, &n, NULL, NULL) != TM_E_INVAL || n < 1 || n > bound) fail("a variant did not name its size", (long)c);
      uint8_t *room = (uint8_t *)exact((size_t)n);
      if (tm_webp_encode_host(frames, w, (int64_t)px, nf, w, h, fps, &other, room, n, &n2, canvas, NULL) != TM_OK || n2 != n) fail("a variant into exact room", (long)c);
      free(room);
      n_variants++;
    }
    free(canvas); free(file); free(want); free(frames);
  }
  fclose(f);
  printf("webp_encode: %ld files of %ld frames equal the restatement's; %ld variants into exact room\n", n_files, n_frames, n_variants);
  return 0;
}
