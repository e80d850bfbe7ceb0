// tm_steps.h -- what tm_steps.hip, tm_reduce.hip and tm_reconstruct.hip need of each other.
#pragma once
#include "tm_encoder.h"

int step_reduce(tm_encoder *e);              // tm_reduce.hip
int step_reconstruct(tm_encoder *e);         // tm_reconstruct.hip
int prefetch_query_features(tm_encoder *e);  // tm_reconstruct.hip: PreparePalettes launches the features of Reconstruct's first queries

// ---- tm_steps.hip ------------------------------------------------------------------------------------------------
int need_frame_tiles(tm_encoder *e, const char *step);
int need_global_rgb(tm_encoder *e, const char *step);
// the query frames [sf, sf + sn) of this process (tm_set_query_shard), inside the clip; true when other frames are left to other processes
bool query_range(const tm_encoder *e, int *sf, int *sn);

// The small shared kernels, on the encoder's stream; every wrapper checks its own launch.
// dst row i = src row idx[i] (rows of 16-byte vectors); dst[i] = src[idx[i]] for T = uint8_t, int32_t, uint32_t
int gather_rows(tm_encoder *e, const void *src, const void *idx, int64_t n, int bytes_per_row, void *dst);
template <class T> int gather(tm_encoder *e, const void *src, const void *idx, int64_t n, void *dst);
// out[i] = idx[i] >= 0 ? table[idx[i]] : -1; in place: negative indices stay as they are
int lookup(tm_encoder *e, const void *idx, int64_t n, const void *table, void *out);
int lookup_inplace(tm_encoder *e, void *idx, int64_t n, const void *table);
int pal_from_tile(tm_encoder *e);  // TMI^.PalIdx := FTiles[TileIdx]^.PalIdx_Initial for every item (1551)

// a buffer of n items, at least one (an empty share still hands a pointer to its kernels and collectives)
inline int alloc_rows(DevBuf &buf, int64_t n, size_t item) { return buf.alloc((size_t)std::max<int64_t>(n, 1) * item); }

// The tile-map arrays over several processes: every process fills the items of its own frames; an item it does not own holds the IDENTITY of
// the array's merge, so that one all-reduce per array leaves every process with every item (tiler_amd/distributed.py merges the same way).
enum { TMA_TILE = 1, TMA_ERR = 2, TMA_PAL = 4, TMA_PM_ERR = 8, TMA_PRED = 16, TMA_PX = 32, TMA_PY = 64 };
int clear_items(tm_encoder *e, int which, int keep_f0 = 0, int keep_nf = 0);  // identity into all items but those of the frames kept
int merge_items(tm_encoder *e, int which);                                    // the all-reduces, in the order of the enum

struct MotionScratch {  // motion search: a frame as a screen of pixels (one or two), the features of its sliding windows and of the current frame's tiles
  DevBuf screen[2], win, cur;
  size_t screen_bytes = 0;
  int alloc(const tm_encoder *e, int nscreens);
};
std::vector<uint8_t> key_frame_mask(const tm_encoder *e);  // [nframes]: 1 where a key frame starts
