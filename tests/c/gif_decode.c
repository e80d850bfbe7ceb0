/* gif_decode.c -- the GIF reader's rule (tm_gif.h, through its host twin in tm_gif_in.hip) under AddressSanitizer /
 * UndefinedBehaviorSanitizer: a stand-alone program (its own main, never loaded into Python, never run on a GPU machine).  The kernels
 * compile the same text, so what is out of bounds here would be out of bounds there.  Every file, every index buffer and every clip sits in
 * an allocation of its exact size:
 *   the cases of tests/gif_cases.py (`python tests/gif_cases.py FILE` writes them): files that decode, files the container walk refuses,
 *   files with a status -- each with the verdict the cases name -- and the seeded damage list, whatever its verdict;
 *   every image's LZW data once more through tm_gif_lzw_streams_host, in a blob that ends with the data and with the span cut short.
 * Build and run: tools/asan_gif_in.sh (this file with clang -fsanitize=address,undefined; tm_gif_in.hip and what it needs with hipcc
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

static long n_calls = 0, n_decoded = 0, n_walk_refused = 0, n_status = 0, n_streams = 0;

static void *exact(size_t n) {
  void *p = malloc(n ? n : 1);
  if (!p) fail("out of memory", (long)n);
  return p;
}

/* one file: the walk, the frame list, the decode into an exact clip, every image's data as a stream of its own.  Returns the walk's code
 * when it refuses, else the first status (>= 0). */
static int run(const uint8_t *data, size_t n) {
  uint8_t *file = (uint8_t *)exact(n);
  if (n) memcpy(file, data, n);
  tm_gif_info info;
  n_calls++;
  int rc = tm_probe_gif_host(file, n, &info);
  if (rc != TM_OK) {
    if (rc != TM_E_IO && rc != TM_E_UNSUPPORTED) fail("the walk refused with another code", rc);
    n_walk_refused++;
    free(file);
    return rc;
  }
  int nf = 0;
  tm_gif_frame *frames = (tm_gif_frame *)exact((size_t)info.frames * sizeof(tm_gif_frame));
  if (tm_gif_frames_host(file, n, frames, info.frames, &nf) != TM_OK || nf != info.frames) fail("tm_gif_frames_host disagrees with the probe", nf);
  const int64_t px = (int64_t)info.width * info.height;
  int first = nf > 2 ? 1 : 0;
  uint32_t *clip = (uint32_t *)exact((size_t)(px * (nf - first)) * 4);
  int32_t *status = (int32_t *)exact((size_t)nf * 4);
  rc = tm_gif_decode_host(file, n, first, nf - first, -1, clip, px, status);
  if (rc != TM_OK) fail("tm_gif_decode_host refused a file its walk accepts", rc);
  int verdict = 0;
  for (int i = 0; i < nf; i++) {
    if (status[i] != 0 && status[i] != TM_GIF_TRUNCATED && status[i] != TM_GIF_BAD_CODE) fail("an unknown status", status[i]);
    if (status[i] && !verdict) verdict = status[i];
  }
  if (verdict) n_status++; else n_decoded++;
  for (int i = 0; i < nf; i++) {  /* the image's data alone, whole and cut, the blob ending where the span ends */
    const tm_gif_frame *f = &frames[i];
    const uint32_t npix = (uint32_t)f->width * (uint32_t)f->height;
    for (int cut = 0; cut < 2; cut++) {
      const size_t len = cut ? (size_t)f->data_bytes / 2 : (size_t)f->data_bytes;
      uint8_t *blob = (uint8_t *)exact(len), *dst = (uint8_t *)exact(npix);
      memcpy(blob, file + f->data_off, len);
      tm_gif_stream st = {0, 0, (uint32_t)len, npix, (uint32_t)f->min_code_size, 0};
      tm_gif_status res;
      if (tm_gif_lzw_streams_host(blob, len, &st, 1, dst, npix, &res) != TM_OK) fail("tm_gif_lzw_streams_host refused a well-formed batch", i);
      if (!cut && res.code != status[i]) fail("the stream's status is not the image's", res.code);
      if (res.out_n > npix || res.in_pos > len) fail("a status outside the stream", (long)res.out_n);
      n_streams++;
      free(blob); free(dst);
    }
  }
  free(status); free(clip); free(frames); free(file);
  return verdict;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 1; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 1; }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) fail("short cases file", 0);
  long n_cases = 0;
  for (uint32_t c = 0; c < count; c++) {
    uint32_t kind = 0, len = 0;
    int32_t code = 0;
    if (fread(&kind, 4, 1, f) != 1 || fread(&code, 4, 1, f) != 1 || fread(&len, 4, 1, f) != 1) fail("short cases file", (long)c);
    uint8_t *data = (uint8_t *)exact(len);
    if (len && fread(data, 1, len, f) != len) fail("short cases file", (long)c);
    const int got = run(data, len);
    if (kind == 0 && got != 0) fail("a good case was refused", (long)c);
    if ((kind == 1 || kind == 2) && got != code) fail("a case did not reach its verdict", (long)c);
    n_cases++;
    free(data);
  }
  fclose(f);
  printf("gif_decode: %ld cases; %ld calls: %ld decoded, %ld with a status, %ld refused by the walk; %ld streams\n", n_cases, n_calls, n_decoded, n_status, n_walk_refused,
         n_streams);
  return 0;
}
