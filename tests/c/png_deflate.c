/* png_deflate.c -- the PNG writer's host twin under AddressSanitizer / UndefinedBehaviorSanitizer: a stand-alone program (its own main,
 * never loaded into Python, never run on a GPU machine).  Every input is held in an allocation of its exact size and every output goes
 * into one of exactly the size the call reported:
 *   tm_deflate_code_lengths_host on random, sparse and Fibonacci frequencies: lengths within the limit, Kraft sum 1;
 *   tm_zlib_compress_host on every length 0 .. 40 over four symbols, runs, noise, and periods at and past the window, then
 *   tm_inflate_host of the result: the input;
 *   tm_png_encode_host at both levels and with every filter on frames whose rows and frames are padded (the last frame's allocation ends
 *   with its last pixel), written to a file and read back with tm_read_png_host: the pixels.
 * Build and run: tools/asan_png_out.sh (this file with clang -fsanitize=address,undefined; tm_deflate.hip, tm_png.hip and tm_tables.hip with
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

static long streams = 0, pictures = 0, codes = 0;

static void check_code(const uint32_t *freq, int nsym, int limit) {
  uint32_t *f = (uint32_t *)malloc((size_t)nsym * 4);
  uint8_t *lens = (uint8_t *)malloc((size_t)nsym);
  memcpy(f, freq, (size_t)nsym * 4);
  if (tm_deflate_code_lengths_host(f, nsym, limit, lens) != TM_OK) fail("code lengths", nsym);
  uint64_t kraft = 0;
  int used = 0;
  for (int s = 0; s < nsym; s++) {
    if (lens[s] > limit) fail("a length beyond the limit", s);
    if (lens[s]) { kraft += 1ull << (limit - lens[s]); used++; }
  }
  if (used < 2 || kraft != 1ull << limit) fail("Kraft sum", used);
  free(f); free(lens);
  codes++;
}

static void check_stream(const uint8_t *data, size_t n) {
  uint8_t *src = (uint8_t *)malloc(n ? n : 1);
  if (n) memcpy(src, data, n);
  int64_t need = 0, got = 0;
  if (tm_zlib_compress_host(n ? src : NULL, (int64_t)n, NULL, 0, &need) != TM_E_INVAL || need < 11) fail("compress: size query", (long)n);
  uint8_t *z = (uint8_t *)malloc((size_t)need);
  if (tm_zlib_compress_host(n ? src : NULL, (int64_t)n, z, need, &got) != TM_OK || got != need) fail("compress", (long)n);
  uint8_t *back = (uint8_t *)malloc(n ? n : 1);
  size_t out_n = 0;
  if (tm_inflate_host(z, (size_t)got, back, n, &out_n) != TM_OK || out_n != n || (n && memcmp(back, src, n))) fail("inflate of the coded stream", (long)n);
  free(src); free(z); free(back);
  streams++;
}

static void check_picture(int w, int h, int nf, int row_pad, int frame_pad, int kind, const char *tmp) {
  const int64_t stride = w + row_pad, frame_px = (int64_t)h * stride + frame_pad, total = (int64_t)(nf - 1) * frame_px + (int64_t)(h - 1) * stride + w;
  uint32_t *px = (uint32_t *)malloc((size_t)total * 4);
  for (int64_t i = 0; i < total; i++) px[i] = 0xffffffffu;
  for (int f = 0; f < nf; f++)
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++) {
        uint32_t c = kind == 0 ? 0x123456u : kind == 1 ? (uint32_t)(((x * 255 / w) << 16) | ((y * 255 / h) << 8) | ((x + y + f) & 255)) : rnd(1u << 24);
        if (kind == 3) c = 0x010101u * (uint32_t)((((x >> 3) + (y >> 3)) * 37 + ((x ^ y) & 3) * 16) & 255);
        px[f * frame_px + y * stride + x] = c;
      }
  int64_t *offs = (int64_t *)malloc((size_t)(nf + 1) * 8);
  for (int level = 0; level <= 1; level++)
    for (int filter = TM_PNG_FILTER_AUTO; filter <= (level ? TM_PNG_FILTER_SMALLER : TM_PNG_FILTER_AUTO); filter++) {
      const tm_png_options opt = {level, filter};
      if (tm_png_encode_host(px, stride, frame_px, nf, w, h, &opt, NULL, 0, offs) != TM_E_INVAL) fail("encode: size query", w);
      const int64_t need = offs[nf];
      int64_t bound = 0;
      if (tm_png_bound_host(w, h, &bound) != TM_OK || need > bound * nf) fail("a file beyond the bound", w);
      uint8_t *out = (uint8_t *)malloc((size_t)need);
      if (tm_png_encode_host(px, stride, frame_px, nf, w, h, &opt, out, need, offs) != TM_OK || offs[nf] != need) fail("encode", w);
      for (int f = 0; f < nf; f++) {
        FILE *fp = fopen(tmp, "wb");
        if (!fp || fwrite(out + offs[f], 1, (size_t)(offs[f + 1] - offs[f]), fp) != (size_t)(offs[f + 1] - offs[f])) fail("cannot write the temporary file", f);
        fclose(fp);
        uint32_t *back = (uint32_t *)malloc((size_t)w * h * 4);
        int gw = 0, gh = 0;
        if (tm_read_png_host(tmp, back, (int64_t)w * h, &gw, &gh) != TM_OK || gw != w || gh != h) fail("read back", f);
        for (int y = 0; y < h; y++)
          for (int x = 0; x < w; x++)
            if (back[(size_t)y * w + x] != (px[f * frame_px + y * stride + x] & 0xffffffu)) fail("pixels differ", y * w + x);
        free(back);
        pictures++;
      }
      free(out);
    }
  free(px); free(offs);
}

int main(int argc, char **argv) {
  const char *tmp = argc > 1 ? argv[1] : "png_deflate_tmp.png";
  /* code lengths */
  uint32_t freq[288];
  for (int round = 0; round < 200; round++) {
    const int nsym = round % 3 == 0 ? 286 : round % 3 == 1 ? 30 : 19, limit = nsym == 19 ? 7 : 15;
    for (int s = 0; s < nsym; s++) freq[s] = rnd(4) ? rnd(1u << (1 + rnd(20))) : 0;
    check_code(freq, nsym, limit);
  }
  for (int s = 0; s < 40; s++) freq[s] = s < 2 ? 1 : freq[s - 1] + freq[s - 2];
  check_code(freq, 40, 15);
  check_code(freq, 19, 7);
  memset(freq, 0, sizeof(freq));
  check_code(freq, 30, 15);
  freq[29] = 3;
  check_code(freq, 30, 15);
  /* streams */
  uint8_t *buf = (uint8_t *)malloc(3 * 32769);
  for (size_t n = 0; n <= 40; n++) {
    for (size_t i = 0; i < n; i++) buf[i] = (uint8_t)rnd(4);
    check_stream(buf, n);
  }
  memset(buf, 7, 3 * 32769);
  check_stream(buf, 259); check_stream(buf, 32768); check_stream(buf, 32769); check_stream(buf, 98304);
  for (size_t period = 32768; period <= 32769; period++) {
    for (size_t i = 0; i < period; i++) buf[i] = (uint8_t)rnd(256);
    memcpy(buf + period, buf, period); memcpy(buf + 2 * period, buf, period);
    check_stream(buf, 3 * period);
  }
  for (size_t i = 0; i < 70000; i++) buf[i] = (uint8_t)(rnd(8) ? "abcdefgh"[i % 7] : rnd(256));
  check_stream(buf, 70000);
  free(buf);
  /* pictures */
  static const int shapes[][2] = {{1, 1}, {5, 3}, {40, 24}, {131, 67}, {264, 136}, {10923, 1}};
  for (unsigned s = 0; s < sizeof(shapes) / sizeof(shapes[0]); s++)
    for (int kind = 0; kind < 4; kind++) check_picture(shapes[s][0], shapes[s][1], kind == 3 ? 3 : 1, kind & 1 ? 5 : 0, kind == 3 ? 11 : 0, kind, tmp);
  remove(tmp);
  printf("png_deflate: %ld codes, %ld streams, %ld pictures ok\n", codes, streams, pictures);
  return 0;
}
