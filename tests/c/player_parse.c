/* player_parse.c -- the .gtm player's host side under AddressSanitizer / UndefinedBehaviorSanitizer: a stand-alone program (its own main,
 * never loaded into Python, never run on a GPU machine).  It writes hand-made streams with tm_write_gtm_host -- every item command: more than
 * 65 536 tiles, more than 1 024 palettes, use-count-1 tiles, short and long offsets, runs of zero offsets, both mirror flags -- then feeds
 * tm_player_probe_host the files and tm_lz_decompress_host / tm_player_parse_host the key frames: intact, cut at every length (small stream) or
 * at many lengths (large one), and with bytes flipped.  Every variant sits in an allocation of its exact size, so a read past its end is
 * seen.  Each call must return TM_OK or a negative code with a message; the intact streams must parse.
 *
 * Build and run: tools/asan_player_parse.sh (the program AND the host code it calls -- tm_player_parse.hip, tm_gtm.hip, tm_lzma.hip, tm_tables.hip -- carry the
 * sanitizers: clang -fsanitize=address,undefined for this file, hipcc -Xarch_host -fsanitize=address,undefined for those; no device is touched).
 * An optional second and further arguments feed one more stream:  player_parse DIR STREAM.lzma TM_W TM_H TILE_COUNT
 * (tests/golden/football_cif_kf1.lzma 44 36 83460).  DESIGN.md section 19 records the result. */
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

static long calls = 0, refused = 0;
static int settle(int rc, const char *what) {  /* a refusal must carry a message */
  calls++;
  if (rc == TM_OK) return 0;
  refused++;
  if (rc > 0 || !tm_last_error() || !tm_last_error()[0]) { fprintf(stderr, "%s: code %d without a message\n", what, rc); exit(2); }
  return rc;
}

/* one parse of n bytes held in an allocation of exactly n bytes */
static int parse_exact(const uint8_t *raw, size_t n, int tm_w, int tm_h, int64_t tiles) {
  uint8_t *copy = (uint8_t *)malloc(n ? n : 1);
  if (n) memcpy(copy, raw, n);
  int frames = 0;
  int64_t nintra = 0;
  int rc = settle(tm_player_parse_host(n ? copy : NULL, n, tm_w, tm_h, tiles, NULL, 0, NULL, 0, NULL, &frames, &nintra), "parse");
  if (rc == TM_OK && frames > 0 && tm_w > 0) {  /* and once more into arrays of exactly the sizes it reported */
    uint64_t *recs = (uint64_t *)malloc((size_t)frames * tm_w * tm_h * 8);
    uint8_t *intra = (uint8_t *)malloc(nintra ? (size_t)nintra * 64 : 1);
    int64_t *first = (int64_t *)malloc(((size_t)frames + 1) * 8);
    rc = settle(tm_player_parse_host(copy, n, tm_w, tm_h, tiles, recs, frames, intra, nintra, first, &frames, &nintra), "parse into arrays");
    if (rc != TM_OK || first[frames] != nintra) { fprintf(stderr, "second parse disagrees\n"); exit(2); }
    free(recs); free(intra); free(first);
  }
  free(copy);
  return rc;
}

static void lz_exact(const uint8_t *src, size_t n, size_t cap) {
  uint8_t *copy = (uint8_t *)malloc(n ? n : 1), *dst = (uint8_t *)malloc(cap ? cap : 1);
  if (n) memcpy(copy, src, n);
  size_t out_n = 0, used = 0;
  settle(tm_lz_decompress_host(copy, n, dst, cap, &out_n, &used), "lz_decompress");
  free(copy); free(dst);
}

static uint8_t *read_file(const char *path, size_t *n) {
  FILE *f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END);
  *n = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t *b = (uint8_t *)malloc(*n ? *n : 1);
  if (fread(b, 1, *n, f) != *n) { fprintf(stderr, "short read of %s\n", path); exit(2); }
  fclose(f);
  return b;
}
static void write_file(const char *path, const uint8_t *b, size_t n) {
  FILE *f = fopen(path, "wb");
  if (!f || fwrite(b, 1, n, f) != n) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
  fclose(f);
}

/* the stream: 5 x 3 items, 9 frames, key frames at 0 and 4; n_shared tiles of use count 2 (the TileSet), then use-count-1 tiles (Intra) */
enum { TM_W = 5, TM_H = 3, PER = TM_W * TM_H, FRAMES = 9, NPAL = 1030 };
static int make_stream(const char *path, int n_shared, int pal_size, int64_t *ntiles_out) {
  const int64_t ntiles = (int64_t)n_shared + 200;
  uint8_t *pal_px = (uint8_t *)calloc((size_t)ntiles, 64);
  uint32_t *use = (uint32_t *)malloc((size_t)ntiles * 4);
  int32_t *palettes = (int32_t *)malloc((size_t)NPAL * pal_size * 4);
  tm_tilemap_item *tm = (tm_tilemap_item *)calloc((size_t)FRAMES * PER, sizeof(tm_tilemap_item));
  for (int64_t t = 0; t < ntiles; t++) {
    use[t] = t < n_shared ? 2 : 1;
    for (int j = 0; j < 64; j++) pal_px[t * 64 + j] = (uint8_t)(((t % 61) * 7 + j * (1 + t % 3)) % pal_size);
  }
  for (int i = 0; i < NPAL * pal_size; i++) palettes[i] = (int32_t)rnd(1u << 24);
  int64_t next_intra = n_shared;
  const int32_t kf[2] = {0, 4};
  for (int f = 0; f < FRAMES; f++)
    for (int i = 0; i < PER; i++) {
      tm_tilemap_item *it = &tm[f * PER + i];
      it->TileIdx = -1; it->PalIdx = -1;
      int kind = (int)rnd(7);
      if (f == 4 && kind >= 4) kind = 0;  /* a key frame starts with drawn items */
      if (kind == 6) {                    /* zero offsets, up to 6 in a row: SkipBlock from 4 on */
        const int n = 2 + (int)rnd(5);
        for (int k = 0; k < n && i < PER; k++, i++) { tm[f * PER + i].TileIdx = -1; tm[f * PER + i].PalIdx = -1; tm[f * PER + i].Flags = 4; }
        i--;
      } else if (kind >= 4) {
        const int wide = (int)rnd(2);
        it->PredictedX = (int8_t)((int)rnd(wide ? 256 : 64) - (wide ? 128 : 32));
        it->PredictedY = (int8_t)((int)rnd(wide ? 256 : 64) - (wide ? 128 : 32));
        it->Flags = 4;
      } else {
        it->Flags = rnd(4);
        it->PalIdx = kind == 2 ? 1024 + (int32_t)rnd(NPAL - 1024) : (int32_t)rnd(1024);
        if (kind == 3) it->TileIdx = (int32_t)next_intra++;
        else it->TileIdx = kind == 1 ? n_shared - 1 - (int32_t)rnd(n_shared > 24 ? 24 : n_shared) : (int32_t)rnd(n_shared > 65536 ? 65536 : n_shared);
      }
    }
  if (next_intra > ntiles) { fprintf(stderr, "too many intra tiles\n"); exit(2); }
  const int rc = tm_write_gtm_host(path, TM_W, TM_H, FRAMES, 25.0, kf, 2, pal_px, use, ntiles, palettes, NPAL, pal_size, tm, "[Load]\r\nInputFileName=made\r\n");
  free(pal_px); free(use); free(palettes); free(tm);
  *ntiles_out = ntiles;
  return rc;
}

/* every key frame of the file at `path`: decode, parse, then the variants (dense: every cut; else cuts around the commands only) */
static void torture(const char *dir, const char *path, int64_t ntiles, int dense) {
  size_t n = 0;
  uint8_t *file = read_file(path, &n);
  tm_gtm_info info;
  int32_t kf[16][4];
  int nkf = 0;
  if (settle(tm_player_probe_host(path, &info, &kf[0][0], 16, &nkf), "probe") != TM_OK || nkf != 2) { fprintf(stderr, "%s: %s\n", path, tm_last_error()); exit(2); }
  /* the file itself: cut short and with header bytes changed */
  char bad[4096];
  snprintf(bad, sizeof(bad), "%s/player_parse_variant.gtm", dir);
  const size_t head = 40 + 28 * (size_t)nkf;
  for (size_t cut = 0; cut <= head + 32 && cut < n; cut++) { write_file(bad, file, cut); settle(tm_player_probe_host(bad, &info, &kf[0][0], 16, &nkf), "probe of a cut file"); }
  for (int k = 0; k < 600; k++) {
    uint8_t *v = (uint8_t *)malloc(n);
    memcpy(v, file, n);
    v[rnd((uint32_t)head)] ^= (uint8_t)(1u << rnd(8));
    write_file(bad, v, n);
    settle(tm_player_probe_host(bad, &info, &kf[0][0], 2, &nkf), "probe of a damaged header");
    free(v);
  }
  remove(bad);
  settle(tm_player_probe_host(path, &info, &kf[0][0], 16, &nkf), "probe");
  size_t pos = head;
  for (int k = 0; k < nkf; k++) {
    const size_t raw_n = (uint32_t)kf[k][1], comp_n = (uint32_t)kf[k][2];
    uint8_t *raw = (uint8_t *)malloc(raw_n + 16);
    size_t out_n = 0, used = 0;
    if (tm_lz_decompress_host(file + pos, comp_n, raw, raw_n + 16, &out_n, &used) != TM_OK || out_n != raw_n) { fprintf(stderr, "key frame %d does not decode\n", k); exit(2); }
    if (parse_exact(raw, raw_n, TM_W, TM_H, ntiles) != TM_OK) { fprintf(stderr, "key frame %d does not parse: %s\n", k, tm_last_error()); exit(2); }
    /* the compressed stream cut short and damaged */
    for (int v = 0; v < (dense ? 300 : 40); v++) lz_exact(file + pos, rnd((uint32_t)comp_n), raw_n + 16);
    for (int v = 0; v < (dense ? 300 : 20); v++) {
      uint8_t *c = (uint8_t *)malloc(comp_n);
      memcpy(c, file + pos, comp_n);
      c[rnd((uint32_t)comp_n)] ^= (uint8_t)(1u << rnd(8));
      lz_exact(c, comp_n, raw_n + 16);
      free(c);
    }
    /* the command bytes cut short: every length, or the lengths around the head and the items */
    const size_t tail = raw_n > 1500 ? raw_n - 1500 : 0;
    for (size_t cut = 0; cut < raw_n; cut++) {
      if (!dense && cut > 200 && cut < tail) { cut = tail; }
      parse_exact(raw, cut, TM_W, TM_H, ntiles);
    }
    /* ... and with a byte changed, in the head or among the items */
    for (int v = 0; v < (dense ? 3000 : 150); v++) {
      uint8_t *c = (uint8_t *)malloc(raw_n);
      memcpy(c, raw, raw_n);
      const size_t at = rnd(4) == 0 || tail == 0 ? rnd((uint32_t)(raw_n < 200 ? raw_n : 200)) : tail + rnd((uint32_t)(raw_n - tail));
      c[at] = rnd(2) ? (uint8_t)(c[at] ^ (1u << rnd(8))) : (uint8_t)rnd(256);
      parse_exact(c, raw_n, TM_W, TM_H, ntiles);
      parse_exact(c, raw_n, 0, 0, 0);  /* (dimensions from the stream itself, where it has them) */
      free(c);
    }
    free(raw);
    pos += comp_n;
  }
  free(file);
}

int main(int argc, char **argv) {
  const char *dir = argc > 1 ? argv[1] : "/tmp";
  char path[4096];
  int64_t ntiles = 0;
  snprintf(path, sizeof(path), "%s/player_parse_small.gtm", dir);
  if (make_stream(path, 48, 2, &ntiles) != TM_OK) { fprintf(stderr, "%s\n", tm_last_error()); return 2; }
  torture(dir, path, ntiles, 1);
  remove(path);
  snprintf(path, sizeof(path), "%s/player_parse_large.gtm", dir);
  if (make_stream(path, 65536 + 24, 64, &ntiles) != TM_OK) { fprintf(stderr, "%s\n", tm_last_error()); return 2; }
  torture(dir, path, ntiles, 0);
  remove(path);
  if (argc >= 6) {  /* one more key frame's compressed stream, e.g. the reference's */
    size_t n = 0;
    uint8_t *blob = read_file(argv[2], &n);
    const int tm_w = atoi(argv[3]), tm_h = atoi(argv[4]);
    const int64_t tiles = atoll(argv[5]);
    size_t out_n = 0, used = 0;
    tm_lz_decompress_host(blob, n, NULL, 0, &out_n, &used);
    uint8_t *raw = (uint8_t *)malloc(out_n + 1);
    if (tm_lz_decompress_host(blob, n, raw, out_n, &out_n, &used) != TM_OK) { fprintf(stderr, "%s: %s\n", argv[2], tm_last_error()); return 2; }
    if (parse_exact(raw, out_n, tm_w, tm_h, tiles) != TM_OK) { fprintf(stderr, "%s: %s\n", argv[2], tm_last_error()); return 2; }
    for (int v = 0; v < 300; v++) parse_exact(raw, rnd((uint32_t)out_n), tm_w, tm_h, tiles);
    for (int v = 0; v < 300; v++) {
      uint8_t *c = (uint8_t *)malloc(out_n);
      memcpy(c, raw, out_n);
      c[rnd((uint32_t)out_n)] ^= (uint8_t)(1u << rnd(8));
      parse_exact(c, out_n, tm_w, tm_h, tiles);
      free(c);
    }
    free(raw); free(blob);
  }
  printf("player_parse: %ld calls, %ld refused with a message, no sanitizer report\n", calls, refused);
  return 0;
}
