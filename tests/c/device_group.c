/* device_group.c -- a plain C host (what a FreePascal host would do) driving several devices from ONE
 * process: tm_set_devices / tm_set_device_mask after tm_create, nothing else changed.  Test infrastructure: built and started as a fresh
 * child process by tests/test_gpu_device_group.py.
 *
 *   device_group single <out>     one encoder                                            -> result dump in <out>
 *   device_group pair <out>       a group of two shards on device 0 (tm_set_devices {0, 0})
 *   device_group all <out>        a group of one shard per visible device (tm_set_device_mask)
 * The dump (the format of native_comm.c) holds every global tile, the palettes and all tile maps: the caller compares dumps byte for byte.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tilemotion.h"

#define W 96
#define H 72
#define F 24

#define CHECK(call)                                                                   \
  do {                                                                                \
    const int rc_ = (call);                                                           \
    if (rc_ != TM_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, tm_last_error()); return 1; } \
  } while (0)

/* a small clip with exact duplicates, near duplicates and a scene cut: gradients that drift, noise from a 64-bit LCG on a quarter
 * of the tiles, every third tile column static */
static void make_clip(uint32_t *px) {
  uint64_t lcg = 0x42381337ull;
  for (int f = 0; f < F; f++)
    for (int y = 0; y < H; y++)
      for (int x = 0; x < W; x++) {
        const int tx = x >> 3, ty = y >> 3;
        const int drift = (tx % 3 == 0) ? 0 : f;
        int r = (x * 255 / W + 2 * drift) & 255, g = (y * 255 / H + drift) & 255, b = ((x + y) * 255 / (W + H) + 3 * drift) & 255;
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        if (((tx * 7 + ty * 13 + f * 5) & 3) == 0) {
          r += (int)((lcg >> 33) % 17) - 8; g += (int)((lcg >> 41) % 17) - 8; b += (int)((lcg >> 49) % 17) - 8;
          r = r < 0 ? 0 : r > 255 ? 255 : r; g = g < 0 ? 0 : g > 255 ? 255 : g; b = b < 0 ? 0 : b > 255 ? 255 : b;
        }
        if (f >= F / 2) { const int t = r; r = g; g = b; b = t; }
        px[((size_t)f * H + y) * W + x] = 0xFF000000u | ((uint32_t)r << 16) | ((uint32_t)g << 8) | (uint32_t)b;
      }
}

static int dump(tm_encoder *e, const char *path) {
  int64_t tiles = 0;
  int frames = 0, palettes = 0, tw = 0, th = 0, kfs = 0;
  CHECK(tm_get_counts(e, &tiles, &frames, &palettes, &tw, &th, &kfs));
  FILE *o = fopen(path, "wb");
  if (!o) { perror(path); return 1; }
  fwrite(&tiles, 8, 1, o); fwrite(&frames, 4, 1, o); fwrite(&palettes, 4, 1, o); fwrite(&kfs, 4, 1, o);
  tm_tile_hdr *hdr = malloc((size_t)tiles * sizeof(tm_tile_hdr));
  uint8_t *pal = malloc((size_t)tiles * 64);
  uint32_t *rgb = malloc((size_t)tiles * 256);
  CHECK(tm_get_tiles(e, 0, tiles, hdr, pal, rgb));
  fwrite(hdr, sizeof(tm_tile_hdr), (size_t)tiles, o); fwrite(pal, 64, (size_t)tiles, o); fwrite(rgb, 256, (size_t)tiles, o);
  int64_t psz = 0;
  CHECK(tm_get_int(e, "PaletteSize", &psz));
  int32_t *pc = malloc((size_t)psz * 4);
  for (int p = 0; p < palettes; p++) { CHECK(tm_get_palette(e, p, pc)); fwrite(pc, 4, (size_t)psz, o); }
  tm_tilemap_item *tm = malloc((size_t)tw * th * sizeof(tm_tilemap_item));
  for (int f = 0; f < frames; f++) { CHECK(tm_get_tilemap(e, f, tm)); fwrite(tm, sizeof(tm_tilemap_item), (size_t)tw * th, o); }
  fclose(o);
  printf("%lld tiles, %d palettes, %d key frames\n", (long long)tiles, palettes, kfs);
  free(hdr); free(pal); free(rgb); free(pc); free(tm);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: device_group single|pair|all <out>\n"); return 2; }
  const int nd = tm_device_count();
  if (nd <= 0) { fprintf(stderr, "no device: %s\n", tm_last_error()); return 3; }
  tm_encoder *e = tm_create();
  if (!e) { fprintf(stderr, "tm_create: %s\n", tm_last_error()); return 1; }
  if (strcmp(argv[1], "pair") == 0) {
    const int devs[2] = {0, 0};
    CHECK(tm_set_devices(e, devs, 2));
  } else if (strcmp(argv[1], "all") == 0) {
    CHECK(tm_set_device_mask(e, nd >= 32 ? 0xffffffffu : (1u << nd) - 1u));
  } else if (strcmp(argv[1], "single") != 0) return 2;
  CHECK(tm_load_default_settings(e));
  CHECK(tm_set_int(e, "PaletteCount", 3));
  CHECK(tm_set_int(e, "MotionPredictRadius", 0));
  CHECK(tm_set_bool(e, "FrameTilingExtendedPaletteUsage", 0));
  CHECK(tm_set_float(e, "ShotTransMinSecondsPerKF", 0.1));
  CHECK(tm_set_video(e, W, H, 24.0, F));
  uint32_t *px = malloc((size_t)F * H * W * 4);
  make_clip(px);
  for (int f = 0; f < F; f++) CHECK(tm_push_frame_rgb32(e, f, px + (size_t)f * H * W, W));
  CHECK(tm_run(e, TM_STEP_ALL));
  if (dump(e, argv[2])) return 1;
  tm_destroy(e);
  free(px);
  return 0;
}
