/* rgb_clip_host.c -- the host side of RGB clips lent in memory under AddressSanitizer / UndefinedBehaviorSanitizer: a stand-alone program (its
 * own main, built by tools/asan_rgb_clip.sh together with the host code it calls; CPU only, no device is touched).  tm_probe_rgb_clip_host
 * and tm_rgb_to_rgb32_host run over every layout on allocations of exactly the described size -- the clip's first sample is the allocation's
 * first byte, its last sample the last byte -- at 1 x 1 and 101 x 53, unscaled and scaled, so that a read of one byte outside the described
 * samples is a report.  The unscaled result is checked against the rule written out here.  Ends with "ok" and no report. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tilemotion.h"

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void) {
  lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(lcg_state >> 33);
}

#define CHECK(x) do { int rc_ = (x); if (rc_ != TM_OK) { fprintf(stderr, "%s:%d: %s -> %d: %s\n", __FILE__, __LINE__, #x, rc_, tm_last_error()); exit(1); } } while (0)

enum { PACKED, PLANAR, GRAY };
typedef struct { const char *name; int kind, nch, idx[3], bytes; } layout;  /* idx: R, G, B among the pixel's channels, or among the planes */
static const layout LAYOUTS[] = {
  {"rgb24", PACKED, 3, {0, 1, 2}, 1}, {"bgr24", PACKED, 3, {2, 1, 0}, 1}, {"rgba", PACKED, 4, {0, 1, 2}, 1}, {"bgra", PACKED, 4, {2, 1, 0}, 1},
  {"argb", PACKED, 4, {1, 2, 3}, 1},  {"abgr", PACKED, 4, {3, 2, 1}, 1},  {"rgb48", PACKED, 3, {0, 1, 2}, 2}, {"bgr48", PACKED, 3, {2, 1, 0}, 2},
  {"rgba64", PACKED, 4, {0, 1, 2}, 2}, {"bgra64", PACKED, 4, {2, 1, 0}, 2}, {"rgbp", PLANAR, 3, {0, 1, 2}, 1}, {"gbrp", PLANAR, 3, {2, 0, 1}, 1},
  {"rgbp16", PLANAR, 3, {0, 1, 2}, 2}, {"gbrp16", PLANAR, 3, {2, 0, 1}, 2}, {"gray", GRAY, 1, {0, 0, 0}, 1}, {"gray16", GRAY, 1, {0, 0, 0}, 2},
};

static int narrow(int word, int samples, int depth) {
  if (samples == TM_SAMPLES_U8) return word;
  const int pd = samples == TM_SAMPLES_U16_LOW ? word & ((1 << depth) - 1) : word >> (16 - depth);
  const int p = (pd + (1 << (depth - 9))) >> (depth - 8);
  return p < 255 ? p : 255;
}

static long clips = 0;

/* one clip of the layout: n frames of w x h, `pad` bytes between rows; the allocation starts at the lowest channel's first sample and ends
 * with the highest channel's last one */
static void one(const layout *L, int samples, int depth, int n, int w, int h, int pad, int dw, int dh) {
  const int B = L->bytes;
  int64_t off[3], step, row, frame;
  if (L->kind == PACKED) {
    int lo = L->idx[0] < L->idx[1] ? L->idx[0] : L->idx[1];
    if (L->idx[2] < lo) lo = L->idx[2];
    step = (int64_t)L->nch * B; row = step * w + pad; frame = row * h;
    for (int i = 0; i < 3; i++) off[i] = (int64_t)(L->idx[i] - lo) * B;
  } else {
    step = B; row = (int64_t)B * w + pad;
    const int64_t plane = row * h;
    frame = plane * (L->kind == PLANAR ? 3 : 1);
    for (int i = 0; i < 3; i++) off[i] = plane * L->idx[i];
  }
  int64_t size = 0;
  for (int i = 0; i < 3; i++) {
    const int64_t end = off[i] + frame * (n - 1) + row * (h - 1) + step * (w - 1) + B;
    if (end > size) size = end;
  }
  uint8_t *buf = (uint8_t *)malloc((size_t)size);
  if (!buf) { perror("malloc"); exit(1); }
  for (int64_t i = 0; i < size; i++) buf[i] = (uint8_t)rnd();
  tm_rgb_clip c;
  memset(&c, 0, sizeof c);
  c.r = buf + off[0]; c.g = buf + off[1]; c.b = buf + off[2];
  c.step = step; c.row = row; c.frame = frame;
  c.width = w; c.height = h; c.frames = n; c.fps = 25.0;
  c.samples = samples; c.depth = depth; c.memory = TM_MEM_HOST;
  int pw = -1, ph = -1;
  CHECK(tm_probe_rgb_clip_host(&c, 1.0, &pw, &ph));
  if (pw != w || ph != h) { fprintf(stderr, "%s: probe says %dx%d for %dx%d\n", L->name, pw, ph, w, h); exit(1); }
  uint32_t *out = (uint32_t *)malloc((size_t)n * dw * dh * sizeof(uint32_t));
  if (!out) { perror("malloc"); exit(1); }
  CHECK(tm_rgb_to_rgb32_host(&c, 0, n, dw, dh, out));
  if (dw == w && dh == h)
    for (int f = 0; f < n; f++)
      for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
          uint32_t want = 0;
          for (int i = 0; i < 3; i++) {
            const uint8_t *s = buf + off[i] + frame * f + row * y + step * x;
            want = want << 8 | (uint32_t)narrow(B == 1 ? s[0] : s[0] | s[1] << 8, samples, depth);
          }
          const uint32_t got = out[((size_t)f * h + y) * w + x];
          if (got != want) { fprintf(stderr, "%s %dx%d depth %d: pixel (%d, %d, %d) is %08x, not %08x\n", L->name, w, h, depth, f, y, x, got, want); exit(1); }
        }
  else
    for (size_t i = 0; i < (size_t)n * dw * dh; i++)
      if (out[i] >> 24) { fprintf(stderr, "%s: a top byte is set\n", L->name); exit(1); }
  if (n > 1) CHECK(tm_rgb_to_rgb32_host(&c, n - 1, 1, dw, dh, out));  /* the last frame alone */
  free(out);
  free(buf);
  clips++;
}

int main(void) {
  for (size_t l = 0; l < sizeof LAYOUTS / sizeof LAYOUTS[0]; l++) {
    const layout *L = &LAYOUTS[l];
    static const int DEEP[][2] = {{TM_SAMPLES_U16_LOW, 9}, {TM_SAMPLES_U16_LOW, 10}, {TM_SAMPLES_U16_LOW, 12}, {TM_SAMPLES_U16_HIGH, 10}, {TM_SAMPLES_U16_HIGH, 16}};
    for (int d = 0; d < (L->bytes == 1 ? 1 : 5); d++) {
      const int samples = L->bytes == 1 ? TM_SAMPLES_U8 : DEEP[d][0], depth = L->bytes == 1 ? 8 : DEEP[d][1];
      for (int pad = 0; pad <= 2; pad += 2) {
        one(L, samples, depth, 1, 1, 1, pad, 1, 1);
        one(L, samples, depth, 2, 1, 1, pad, 3, 2);
        one(L, samples, depth, 2, 101, 53, pad, 101, 53);
        one(L, samples, depth, 2, 101, 53, pad, 76, 40);
        one(L, samples, depth, 1, 101, 53, pad, 150, 78);
        one(L, samples, depth, 1, 40, 24, pad, 5, 3);
      }
    }
  }
  /* refusals come back as codes with a message, and read nothing */
  tm_rgb_clip bad;
  memset(&bad, 0, sizeof bad);
  int w = 0, h = 0;
  if (tm_probe_rgb_clip_host(NULL, 1.0, &w, &h) != TM_E_INVAL || tm_probe_rgb_clip_host(&bad, 1.0, &w, &h) != TM_E_INVAL || !*tm_last_error()) {
    fprintf(stderr, "a null clip is not refused\n");
    return 1;
  }
  printf("ok: %ld clips\n", clips);
  return 0;
}
