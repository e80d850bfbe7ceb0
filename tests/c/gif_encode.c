/* gif_encode.c -- the GIF writer's rule (tm_gif_out.h, through its host twin in tm_gif_out.hip) under AddressSanitizer /
 * UndefinedBehaviorSanitizer: a stand-alone program (its own main, never loaded into Python, never run on a GPU machine).  The kernels
 * compile the same text (lzw_segment, the tables' layout), so what is out of bounds here would be out of bounds there.  Every clip, every
 * file and every canvas sits in an allocation of its exact size:
 *   the clips of tests/gif_out_cases.py (`python tests/gif_out_cases.py FILE` writes them with the restatement's files): the twin's file
 *   must be the restatement's byte for byte, into room of exactly that size; one byte less must be refused with the size and write
 *   nothing; tm_gif_bound_host must bound it; the project's reader (tm_gif_decode_host) must show the canvas the twin returns;
 *   every clip's first frame once more through tm_gif_palettise_host and its indices through tm_gif_lzw_pack_host at three segment sizes.
 * Build and run: tools/asan_gif_out.sh (this file with clang -fsanitize=address,undefined; tm_gif_out.hip and what it needs with hipcc
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

static long n_files = 0, n_frames = 0, n_payloads = 0;

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
    tm_gif_options opt = {o[0], o[1], o[2], o[3], o[4], o[5]};

    int64_t bound = 0, need = -1;
    if (tm_gif_bound_host(w, h, nf, &opt, &bound) != TM_OK || bound < (int64_t)want_n) fail("the bound does not hold the file", (long)c);
    uint8_t *file = (uint8_t *)exact(want_n);
    uint32_t *canvas = (uint32_t *)exact(px * nf * 4);
    tm_gif_export_stats st;
    if (tm_gif_encode_host(frames, w, (int64_t)px, nf, w, h, fps, &opt, file, (int64_t)want_n - 1, &need, NULL, NULL) != TM_E_INVAL || need != (int64_t)want_n)
      fail("room one byte short was not refused with the size", (long)c);
    if (tm_gif_encode_host(frames, w, (int64_t)px, nf, w, h, fps, &opt, file, want_n, &need, canvas, &st) != TM_OK) fail("the twin refused a case", (long)c);
    if (need != (int64_t)want_n || memcmp(file, want, want_n)) fail("the twin's file is not the restatement's", (long)c);
    if (st.frames != nf || st.file_bytes != (int64_t)want_n) fail("the stats disagree", (long)c);
    uint32_t *shown = (uint32_t *)exact(px * nf * 4);
    int32_t *status = (int32_t *)exact((size_t)nf * 4);
    if (tm_gif_decode_host(file, want_n, 0, nf, -1, shown, (int64_t)px, status) != TM_OK) fail("the reader refused the file", (long)c);
    for (int i = 0; i < nf; i++) if (status[i]) fail("the reader met a status", status[i]);
    if (memcmp(shown, canvas, px * nf * 4)) fail("the reader does not show the twin's canvas", (long)c);
    n_files++; n_frames += nf;

    uint32_t table[256];
    int colours = 0, is_exact = 0;
    uint8_t *idx = (uint8_t *)exact(px);
    if (o[0] != TM_GIF_COLOURS_EXACT) {
      if (tm_gif_palettise_host(frames, w, w, h, &opt, table, &colours, &is_exact, idx) != TM_OK || colours < 1 || colours > opt.max_colours) fail("palettise", (long)c);
      int min_code = 2;
      while ((1 << min_code) < colours) min_code++;
      const int segs[3] = {0, 256, 1000};
      for (int s = 0; s < 3; s++) {
        int64_t n = -1;
        if (tm_gif_lzw_pack_host(idx, (uint32_t)px, min_code, segs[s], NULL, 0, &n) != TM_E_INVAL || n < 1) fail("lzw pack did not name its size", (long)c);
        uint8_t *payload = (uint8_t *)exact((size_t)n);
        int64_t n2 = -1;
        if (tm_gif_lzw_pack_host(idx, (uint32_t)px, min_code, segs[s], payload, n, &n2) != TM_OK || n2 != n) fail("lzw pack into exact room", (long)c);
        free(payload);
        n_payloads++;
      }
    }
    free(idx); free(status); free(shown); free(canvas); free(file); free(want); free(frames);
  }
  fclose(f);
  printf("gif_encode: %ld files of %ld frames equal the restatement's and read back; %ld payloads\n", n_files, n_frames, n_payloads);
  return 0;
}
