/* jpeg_encode.c -- the JPEG writer's host twin under AddressSanitizer / UndefinedBehaviorSanitizer: a stand-alone program (its own main,
 * never loaded into Python, never run on a GPU machine).  Its input is the file tests/jpeg_out_cases.py writes: pictures with their
 * options and the files the Python restatement makes of them.  Every picture is held in an allocation of its exact size and every output
 * goes into one of exactly the size the call reported:
 *   tm_jpeg_encode_host with no room at all: TM_E_INVAL, the bytes needed, which are the restatement's and within tm_jpeg_bound_host;
 *   with one byte less than needed: the same, and the buffer is not touched; with exactly the bytes needed: the restatement's file;
 *   the file through tm_jpeg_decode_host: status 0;
 *   three frames whose rows and frames are padded (the allocation ends with the last frame's last pixel): three times that file;
 *   tm_jpeg_quant_tables_host at every quality, and the refusals.
 * Build and run: tools/asan_jpeg_out.sh (this file with clang -fsanitize=address,undefined; tm_jpeg_out.hip, tm_jpeg_in.hip and
 * tm_tables.hip with hipcc -Xarch_host -fsanitize=address,undefined; no device is touched). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tilemotion.h"

static void fail(const char *what, long n) {
  fprintf(stderr, "%s (%ld): %s\n", what, n, tm_last_error() ? tm_last_error() : "");
  exit(2);
}

static long encodes = 0, decodes = 0, refusals = 0, tables = 0;

static void check_item(long item, int w, int h, const tm_jpeg_options *opt, const uint32_t *pixels, const uint8_t *want, int64_t want_n) {
  const size_t npx = (size_t)w * h;
  uint32_t *px = (uint32_t *)malloc(npx * 4);
  memcpy(px, pixels, npx * 4);
  int64_t offs[4] = {-1, -1, -1, -1}, bound = 0;
  if (tm_jpeg_encode_host(px, w, (int64_t)npx, 1, w, h, opt, NULL, 0, offs) != TM_E_INVAL || offs[1] != want_n) fail("encode: size query", item);
  if (tm_jpeg_bound_host(w, h, opt, &bound) != TM_OK || want_n > bound) fail("a file beyond the bound", item);
  uint8_t *out = (uint8_t *)malloc((size_t)want_n);
  memset(out, 0x5a, (size_t)want_n);
  if (tm_jpeg_encode_host(px, w, (int64_t)npx, 1, w, h, opt, out, want_n - 1, offs) != TM_E_INVAL || offs[1] != want_n) fail("encode: a byte short", item);
  for (int64_t i = 0; i < want_n - 1; i++) if (out[i] != 0x5a) fail("a refused call wrote", item);
  if (tm_jpeg_encode_host(px, w, (int64_t)npx, 1, w, h, opt, out, want_n, offs) != TM_OK || offs[0] != 0 || offs[1] != want_n) fail("encode", item);
  if (memcmp(out, want, (size_t)want_n)) fail("the file differs from the restatement's", item);
  encodes += 3;
  /* back through the reader's host form, planes of the exact size */
  const int cw = w, ch = h;  /* (a plane's slot: the picture's size, whatever the sampling) */
  uint8_t *planes[3];
  for (int c = 0; c < 3; c++) planes[c] = (uint8_t *)malloc((size_t)cw * ch);
  const int64_t strides[6] = {cw, (int64_t)cw * ch, cw, (int64_t)cw * ch, cw, (int64_t)cw * ch};
  const void *files[1] = {out};
  const size_t sizes[1] = {(size_t)want_n};
  int32_t status = -1;
  if (tm_jpeg_decode_host(files, sizes, 1, w, h, planes[0], planes[1], planes[2], strides, &status) != TM_OK || status != 0) fail("decode of the file", item);
  decodes++;
  for (int c = 0; c < 3; c++) free(planes[c]);
  /* three padded frames; the allocation ends with the last pixel */
  const int64_t stride = w + 3, frame_px = (int64_t)h * stride + 5, total = 2 * frame_px + (int64_t)(h - 1) * stride + w;
  uint32_t *three = (uint32_t *)malloc((size_t)total * 4);
  for (int64_t i = 0; i < total; i++) three[i] = 0x00fe01fdu;
  for (int f = 0; f < 3; f++)
    for (int y = 0; y < h; y++) memcpy(three + f * frame_px + y * stride, pixels + (size_t)y * w, (size_t)w * 4);
  uint8_t *out3 = (uint8_t *)malloc((size_t)want_n * 3);
  if (tm_jpeg_encode_host(three, stride, frame_px, 3, w, h, opt, out3, want_n * 3, offs) != TM_OK || offs[3] != want_n * 3) fail("encode of three frames", item);
  for (int f = 0; f < 3; f++) if (offs[f] != want_n * f || memcmp(out3 + offs[f], want, (size_t)want_n)) fail("a padded frame's file differs", item);
  encodes++;
  free(three); free(out3); free(out); free(px);
}

static void expect_refused(int rc, const char *what) {
  if (rc != TM_E_INVAL) fail(what, rc);
  refusals++;
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: jpeg_encode CASES.bin\n"); return 2; }
  FILE *fp = fopen(argv[1], "rb");
  if (!fp) fail("cannot open the cases", 0);
  uint32_t count = 0;
  if (fread(&count, 4, 1, fp) != 1) fail("short cases file", 0);
  for (uint32_t i = 0; i < count; i++) {
    uint32_t hd[6];
    if (fread(hd, 4, 6, fp) != 6) fail("short cases file", i);
    const size_t npx = (size_t)hd[0] * hd[1];
    uint32_t *pixels = (uint32_t *)malloc(npx * 4);
    uint8_t *want = (uint8_t *)malloc(hd[5]);
    if (fread(pixels, 4, npx, fp) != npx || fread(want, 1, hd[5], fp) != hd[5]) fail("short cases file", i);
    const tm_jpeg_options opt = {(int32_t)hd[2], (int32_t)hd[3], (int32_t)hd[4]};
    check_item(i, (int)hd[0], (int)hd[1], &opt, pixels, want, hd[5]);
    free(pixels); free(want);
  }
  fclose(fp);
  /* the quantisers: within 1 .. 255, and all ones at quality 100 */
  uint16_t *luma = (uint16_t *)malloc(128), *chroma = (uint16_t *)malloc(128);
  for (int q = 1; q <= 100; q++) {
    if (tm_jpeg_quant_tables_host(q, luma, chroma) != TM_OK) fail("quant tables", q);
    for (int k = 0; k < 64; k++) if (luma[k] < 1 || luma[k] > 255 || chroma[k] < 1 || chroma[k] > 255 || (q == 100 && (luma[k] != 1 || chroma[k] != 1))) fail("a quantiser", q);
    tables++;
  }
  /* refusals: nothing is read or written */
  uint32_t *px = (uint32_t *)malloc(16 * 4);
  memset(px, 0, 64);
  int64_t offs[3] = {-7, -7, -7}, bound = 0;
  uint8_t *out = (uint8_t *)malloc(16);
  const tm_jpeg_options good = {90, TM_JPEG_420, 1}, q0 = {0, 0, 1}, q101 = {101, 0, 1}, s4 = {90, 4, 1}, r1 = {90, 0, -1}, wide = {90, TM_JPEG_444, 16};
  expect_refused(tm_jpeg_encode_host(px, 4, 16, 1, 4, 4, NULL, out, 16, offs), "null options");
  expect_refused(tm_jpeg_encode_host(px, 4, 16, 1, 4, 4, &q0, out, 16, offs), "quality 0");
  expect_refused(tm_jpeg_encode_host(px, 4, 16, 1, 4, 4, &q101, out, 16, offs), "quality 101");
  expect_refused(tm_jpeg_encode_host(px, 4, 16, 1, 4, 4, &s4, out, 16, offs), "sampling 4");
  expect_refused(tm_jpeg_encode_host(px, 4, 16, 1, 4, 4, &r1, out, 16, offs), "restart_rows -1");
  expect_refused(tm_jpeg_encode_host(px, 4, 16, 1, 0, 4, &good, out, 16, offs), "width 0");
  expect_refused(tm_jpeg_encode_host(px, 4, 16, 1, 4, 32769, &good, out, 16, offs), "height 32769");
  expect_refused(tm_jpeg_encode_host(px, 32768, 32768, 0, 32768, 1, &wide, out, 16, offs), "a restart interval of 65536 MCUs");
  expect_refused(tm_jpeg_encode_host(px, 3, 16, 1, 4, 4, &good, out, 16, offs), "a short row stride");
  expect_refused(tm_jpeg_encode_host(px, 4, 15, 2, 4, 4, &good, out, 16, offs), "a short frame stride");
  expect_refused(tm_jpeg_encode_host(px, 4, 16, -1, 4, 4, &good, out, 16, offs), "-1 frames");
  expect_refused(tm_jpeg_encode_host(NULL, 4, 16, 1, 4, 4, &good, out, 16, offs), "null frames");
  expect_refused(tm_jpeg_encode_host(px, 4, 16, 1, 4, 4, &good, out, 16, NULL), "null offsets");
  expect_refused(tm_jpeg_encode_host(px, 4, 16, 1, 4, 4, &good, NULL, 16, offs), "null out with room");
  if (offs[0] != -7 || offs[1] != -7 || offs[2] != -7) fail("a refusal wrote the offsets", 0);
  expect_refused(tm_jpeg_bound_host(4, 4, &good, NULL), "bound: null");
  expect_refused(tm_jpeg_bound_host(4, 4, &q0, &bound), "bound: quality 0");
  expect_refused(tm_jpeg_quant_tables_host(0, luma, chroma), "tables: quality 0");
  expect_refused(tm_jpeg_quant_tables_host(50, NULL, chroma), "tables: null");
  free(px); free(out); free(luma); free(chroma);
  printf("jpeg_encode: %u pictures, %ld encode calls, %ld decodes, %ld quantiser tables, %ld refusals ok\n", count, encodes, decodes, tables, refusals);
  return 0;
}
