// tm_player.h -- what the player's files share (tm_player.hip: the object and tm_player_*; tm_player_parse.hip: its host side, no device
// call; tm_play_frame.hip: the kernel); nobody else includes it.
#pragma once
#include <chrono>
#include <string>
#include <vector>

#include "tm_common.h"
#include "tm_gtm.h"

namespace tmx {

// ---- the record of one tile-map item (tilemotion.h, tm_player_parse_host, describes it for callers)
struct PlayRec {
  uint32_t a;      // tile index | intra: index among the frame's intra tiles | predicted: (uint8) x | (uint8) y << 8
  uint16_t pal;
  uint8_t flags;   // bit 0 H mirror, bit 1 V mirror, bit 2 predicted, bit 3 intra
  uint8_t zero;
};
static_assert(sizeof(PlayRec) == 8, "record layout");
constexpr uint8_t REC_PRED = 4, REC_INTRA = 8;

// ---- header and index
struct KfEntry { int32_t frame; uint32_t raw, comp, ms; int64_t offset; };
static_assert(sizeof(KfEntry) == 24, "the index in memory: 24 bytes per key frame (tm_player_info's host_bytes counts it)");
struct GtmIndex {
  int32_t width = 0, height = 0, frames = 0, version = 0;
  uint32_t avg = 0, kf_max = 0;
  std::vector<KfEntry> kf;
  int kf_frames(int k) const { return (k + 1 < (int)kf.size() ? kf[(size_t)k + 1].frame : frames) - kf[(size_t)k].frame; }
};

// ---- the command stream into records
constexpr int64_t MAX_ITEMS = (int64_t)1 << 24;  // items of a frame the player takes: a gigapixel picture, 128 MB of records a frame; beyond it a SetDimensions is damage
struct StreamHead {  // what the first key frame says about the whole stream
  int want_w = 0, want_h = 0;  // the GTMv header's picture size, which SetDimensions must match (0: no header at hand, tm_player_parse_host)
  bool have_dims = false;
  int tm_w = 0, tm_h = 0, pal_size = 0;
  uint32_t frame_ns = 0;
  int64_t tile_count = 0;
  std::string settings;
  std::vector<uint8_t> tileset;    // [tileset_tiles][64]: tiles drawn by index
  std::vector<int32_t> palettes;   // [pal_count][pal_size] 0x00BBGGRR
  int64_t tileset_tiles() const { return (int64_t)(tileset.size() / 64); }
  int pal_count() const { return pal_size > 0 ? (int)(palettes.size() / (size_t)pal_size) : 0; }
};
struct KfRecords {
  int index = -1, first = 0, nframes = 0;
  std::vector<PlayRec> recs;           // [nframes][tm_w * tm_h]
  std::vector<uint8_t> intra;          // the frames' intra tiles, 64 bytes each, in item order
  std::vector<int64_t> intra_first;    // [nframes + 1]
  double decode_ms = 0, parse_ms = 0;
  std::string err;
  size_t bytes() const { return recs.size() * sizeof(PlayRec) + intra.size() + intra_first.size() * sizeof(int64_t); }
};

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// tm_player_parse.hip (host only)
int read_index(int fd, const char *path, GtmIndex *ix);
// Key frame k of the indexed file: read, decoded and walked into records.  Any thread: reads only the index and, for k > 0, the head's
// dimensions; key frame 0 fills the head (keeps_head false: read again after a seek -- the caller holds the head already).  A failure's
// message is left in out->err as well: a worker thread's message is its own.
int load_keyframe(int fd, const char *path, const GtmIndex &ix, int k, StreamHead *head, bool keeps_head, KfRecords *out);
// A stream's head: the file opened (*fd is the caller's to close, also after a failure), its index, and key frame 0 into head and first.
// Every refusal of a stream is decided here, with no device call.
int open_stream_head(const char *path, int *fd, GtmIndex *ix, StreamHead *head, KfRecords *first);
int fill_info(const GtmIndex &ix, const StreamHead &h, int64_t tileset_tiles, int pal_count, tm_gtm_info *o);
// tm_play_frame.hip
int launch_play_frame(const void *recs, const void *intra, int64_t nintra, const void *tiles, int64_t ntiles, const void *palettes, int npal, int pal_size,
                      const void *prev, void *out, int tm_w, int tm_h, hipStream_t stream);

}  // namespace tmx
