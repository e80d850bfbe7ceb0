// tm_player_parse.hip -- the player's host side, with no device call: a .gtm file's header and index, a key frame's command stream into
// item records, and the head of a stream as tm_player_open and probe_gtm both take it.
//
// Per key frame: the compressed stream is read from the file at its index entry's offset, decoded (lz_decompress), and walked
// (walk_gtm_keyframe, tm_gtm_walk.h: the grammar tm_reload_gtm reads by) into fixed-size records -- 8 bytes per tile-map item, and the
// 64 index bytes of every intra item, which travel with the frame that draws them, so no table of intra slots exists.
// This is the strict reader: what it does not play it refuses here (tilemotion.h lists the codes).
#include <fcntl.h>
#include <unistd.h>

#include "tm_gtm_walk.h"
#include "tm_input.h"
#include "tm_player.h"

namespace tmx {

// the header and one entry per key frame (tm_gtm.h; tilingencoder.pas:30-51), every field checked; every stream must lie inside the file
int read_index(int fd, const char *path, GtmIndex *ix) {
  const int64_t fsize = lseek(fd, 0, SEEK_END);
  uint8_t h[GTM_HEADER_BYTES];
  TM_CHECK(fsize >= 4 && pread_all(fd, h, 4, 0) == 0, TM_E_IO, "%s: too short to be a .gtm file", path);
  if (!gtm_has_magic(h, GTM_HEADER_MAGIC)) {
    set_error("%s has no GTMv header: a headerless stream has no index, so no seek and no frame count (tm_reload_gtm reads those)", path);
    return TM_E_UNSUPPORTED;
  }
  TM_CHECK(fsize >= (int64_t)GTM_HEADER_BYTES && pread_all(fd, h, GTM_HEADER_BYTES, 0) == 0, TM_E_IO, "%s: truncated GTMv header", path);
  const GtmHeader g = decode_gtm_header(h);
  const uint32_t whole = g.whole_header_size, nkf = g.kf_count, frames = g.frame_count;
  ix->version = (int32_t)g.encoder_version; ix->width = (int32_t)g.width; ix->height = (int32_t)g.height;
  ix->avg = g.avg_bytes_per_s; ix->kf_max = g.kf_max_bytes_per_s;
  TM_CHECK(g.riff_size == GTM_HEADER_RIFF && nkf >= 1 && nkf <= (1u << 24) && (uint64_t)whole == GTM_HEADER_BYTES + GTM_KF_BYTES * (uint64_t)nkf && (int64_t)whole <= fsize,
           TM_E_IO, "%s: damaged GTMv header (%u key frames, header of %u bytes, file of %lld)", path, nkf, whole, (long long)fsize);
  TM_CHECK(frames >= nkf && frames <= 0x7fffffffu && ix->width > 0 && ix->height > 0 && ix->width <= 65536 * 8 && ix->height <= 65536 * 8, TM_E_IO,
           "%s: damaged GTMv header (%u frames in %u key frames, %d x %d)", path, frames, nkf, ix->width, ix->height);
  ix->frames = (int32_t)frames;
  std::vector<uint8_t> raw((size_t)nkf * GTM_KF_BYTES);
  TM_CHECK(pread_all(fd, raw.data(), raw.size(), (int64_t)GTM_HEADER_BYTES) == 0, TM_E_IO, "%s: truncated GTMk index", path);
  ix->kf.resize(nkf);
  int64_t off = whole;
  for (uint32_t k = 0; k < nkf; k++) {
    const uint8_t *e = raw.data() + (size_t)k * GTM_KF_BYTES;
    const GtmKfEntry ge = decode_gtm_kf_entry(e);
    KfEntry &d = ix->kf[k];
    d.frame = (int32_t)ge.frame; d.raw = ge.raw_size; d.comp = ge.comp_size; d.ms = ge.time_ms; d.offset = off;
    TM_CHECK(gtm_has_magic(e, GTM_KF_MAGIC) && ge.riff_size == GTM_KF_RIFF && ge.index == k, TM_E_IO, "%s: damaged GTMk entry %u", path, k);
    TM_CHECK(k == 0 ? d.frame == 0 : (d.frame > ix->kf[k - 1].frame && (uint32_t)d.frame < frames), TM_E_IO, "%s: GTMk entry %u starts at frame %d", path, k, d.frame);
    TM_CHECK(d.comp >= 18 && off + (int64_t)d.comp <= fsize, TM_E_IO, "%s: key frame %u (%u bytes at %lld) runs past the file's %lld bytes", path, k, d.comp,
             (long long)off, (long long)fsize);
    off += d.comp;
  }
  return TM_OK;
}

namespace {

// ---- the command stream into records ---------------------------------------------------------------------------------------------------
struct RecordSink {
  StreamHead *head;
  bool takes_head;  // the first key frame: SetDimensions, TileSet, LoadPalette and the settings text are taken; later ones must not bring any
  bool keeps_head;  // ... and kept (false: the first key frame read again after a seek -- the player holds them already)
  int max_frames;   // the frames the index gives this key frame: more is a damaged stream, not a reason to grow
  KfRecords *kf;
  int tm_pos = 0;
  bool frame_open = false;

  int per() const { return head->tm_w * head->tm_h; }
  int place(PlayRec r, const char *what) {
    TM_CHECK(head->have_dims && tm_pos < per(), TM_E_IO, "%s past the tile map", what);
    if (!frame_open) {
      TM_CHECK(kf->nframes < max_frames, TM_E_IO, "more frames in the key frame than the %d its index entry gives it", max_frames);
      kf->recs.resize(kf->recs.size() + (size_t)per());
      if (kf->intra_first.empty()) kf->intra_first.push_back(0);
      frame_open = true;
    }
    kf->recs[kf->recs.size() - (size_t)per() + tm_pos] = r;
    tm_pos++;
    return TM_OK;
  }
  int settings(uint32_t kind, const uint8_t *text, size_t n) {
    if (!(takes_head && keeps_head && kind == 0)) return TM_OK;
    take_settings_text(text, n, &head->settings, &head->pal_size);
    return TM_OK;
  }
  int dimensions(int tm_w, int tm_h, uint32_t ns, uint32_t tc) {
    if (head->have_dims) {
      TM_CHECK(tm_w == head->tm_w && tm_h == head->tm_h && (int64_t)tc == head->tile_count, TM_E_IO, "SetDimensions changes the stream's %d x %d, %lld tiles",
               head->tm_w, head->tm_h, (long long)head->tile_count);
      return TM_OK;
    }
    TM_CHECK(takes_head, TM_E_IO, "SetDimensions outside the first key frame");
    TM_CHECK(head->want_w == 0 || ((int64_t)tm_w * 8 == head->want_w && (int64_t)tm_h * 8 == head->want_h), TM_E_IO,
             "SetDimensions' %d x %d tiles are not the GTMv header's %d x %d pixels", tm_w, tm_h, head->want_w, head->want_h);
    TM_CHECK((int64_t)tm_w * tm_h <= MAX_ITEMS, TM_E_IO, "SetDimensions' %d x %d tiles: more than %lld items a frame", tm_w, tm_h, (long long)MAX_ITEMS);
    head->tm_w = tm_w; head->tm_h = tm_h; head->frame_ns = ns; head->tile_count = tc; head->have_dims = true;
    return TM_OK;
  }
  int pal_size() const { return head->pal_size; }
  int tile_set(int pal_size, uint32_t a, uint32_t b, const uint8_t *px) {
    if (!takes_head) { set_error("a TileSet outside the first key frame is not played (tm_reload_gtm reads such streams)"); return TM_E_UNSUPPORTED; }
    if (!keeps_head) return TM_OK;
    TM_CHECK(head->have_dims && (int64_t)b < head->tile_count, TM_E_IO, "tile set [%u, %u] beyond the declared tile count %lld", a, b, (long long)head->tile_count);
    if ((int64_t)a > head->tileset_tiles()) { set_error("a TileSet that leaves a gap (starts at %u after %lld tiles) is not played", a, (long long)head->tileset_tiles()); return TM_E_UNSUPPORTED; }
    if (head->tileset.size() < ((size_t)b + 1) * 64) head->tileset.resize(((size_t)b + 1) * 64);
    memcpy(&head->tileset[(size_t)a * 64], px, ((size_t)b - a + 1) * 64);
    head->pal_size = pal_size;
    return TM_OK;
  }
  int load_palette(uint32_t pi, const uint8_t *c) {
    if (!takes_head) { set_error("a LoadPalette outside the first key frame is not played (tm_reload_gtm reads such streams)"); return TM_E_UNSUPPORTED; }
    if (!keeps_head) return TM_OK;
    const size_t ps = (size_t)head->pal_size;
    if ((size_t)pi > (size_t)head->pal_count()) { set_error("a LoadPalette that leaves a gap (palette %u after %d) is not played", pi, head->pal_count()); return TM_E_UNSUPPORTED; }
    if (head->palettes.size() < ((size_t)pi + 1) * ps) head->palettes.resize(((size_t)pi + 1) * ps, 0);
    take_palette_words(c, ps, head->palettes.data() + (size_t)pi * ps);
    return TM_OK;
  }
  int frame_end(bool) {
    TM_CHECK(head->have_dims && tm_pos == per(), TM_E_IO, "incomplete tile map at FrameEnd (%d of %d items)", tm_pos, head->have_dims ? per() : 0);
    tm_pos = 0;
    frame_open = false;
    kf->nframes++;
    kf->intra_first.push_back((int64_t)(kf->intra.size() / 64));
    return TM_OK;
  }
  int skip(uint32_t count) {
    for (uint32_t k = 0; k < count; k++) TM_TRY(place(PlayRec{0, 0, REC_PRED, 0}, "SkipBlock"));
    return TM_OK;
  }
  int predicted(int ox, int oy) { return place(PlayRec{(uint32_t)(uint8_t)ox | ((uint32_t)(uint8_t)oy << 8), 0, REC_PRED, 0}, "a predicted item"); }
  int drawn(uint32_t tile, uint32_t pal, uint32_t mirror) { return place(PlayRec{tile, (uint16_t)pal, (uint8_t)mirror, 0}, "a tile-map item"); }
  int intra(uint32_t pal, uint32_t mirror, const uint8_t *px) {
    const int64_t in_frame = (int64_t)(kf->intra.size() / 64) - (kf->intra_first.empty() ? 0 : kf->intra_first.back());
    TM_TRY(place(PlayRec{(uint32_t)in_frame, (uint16_t)pal, (uint8_t)(mirror | REC_INTRA), 0}, "an intra item"));
    kf->intra.insert(kf->intra.end(), px, px + 64);
    return TM_OK;
  }
};

int parse_keyframe(const uint8_t *raw, size_t n, const char *name, StreamHead *head, bool takes_head, bool keeps_head, int max_frames, KfRecords *kf) {
  kf->recs.clear(); kf->intra.clear(); kf->intra_first.clear();
  kf->nframes = 0;
  RecordSink sink{head, takes_head, keeps_head, max_frames, kf};
  TM_TRY(walk_gtm_keyframe(raw, n, name, sink));
  if (kf->intra_first.empty()) kf->intra_first.push_back(0);
  return TM_OK;
}

}  // namespace

int load_keyframe(int fd, const char *path, const GtmIndex &ix, int k, StreamHead *head, bool keeps_head, KfRecords *out) {
  const KfEntry &e = ix.kf[(size_t)k];
  std::vector<uint8_t> comp(e.comp), raw;
  int rc = TM_OK;
  auto fail = [&](int code) { out->err = get_error(); return code; };
  if (pread_all(fd, comp.data(), comp.size(), e.offset) != 0) { set_error("%s: cannot read key frame %d", path, k); return fail(TM_E_IO); }
  double t0 = now_ms();
  size_t used_bytes = 0;
  rc = lz_decompress(comp.data(), comp.size(), raw, &used_bytes, (size_t)e.raw + 1);  // (one more than the index says: enough to see that it is wrong)
  if (rc != TM_OK) { set_error("%s: key frame %d: %s", path, k, std::string(get_error()).c_str()); return fail(TM_E_IO); }
  out->decode_ms = now_ms() - t0;
  if (raw.size() != e.raw) { set_error("%s: key frame %d decodes to %zu bytes, its GTMk entry says %u", path, k, raw.size(), e.raw); return fail(TM_E_IO); }
  t0 = now_ms();
  rc = parse_keyframe(raw.data(), raw.size(), path, head, k == 0, keeps_head, ix.kf_frames(k), out);
  out->parse_ms = now_ms() - t0;
  if (rc != TM_OK) return fail(rc);
  if (out->nframes != ix.kf_frames(k)) { set_error("%s: key frame %d holds %d frames, the index says %d", path, k, out->nframes, ix.kf_frames(k)); return fail(TM_E_IO); }
  out->index = k; out->first = e.frame;
  return TM_OK;
}

int open_stream_head(const char *path, int *fd, GtmIndex *ix, StreamHead *head, KfRecords *first) {
  *fd = open(path, O_RDONLY);
  TM_CHECK(*fd >= 0, TM_E_IO, "cannot open %s", path);
  TM_TRY(read_index(*fd, path, ix));
  head->want_w = ix->width; head->want_h = ix->height;
  const int rc = load_keyframe(*fd, path, *ix, 0, head, true, first);
  if (rc != TM_OK) { set_error("%s", first->err.c_str()); return rc; }
  TM_CHECK(head->have_dims, TM_E_IO, "%s: the first key frame has no SetDimensions", path);
  return TM_OK;
}

int fill_info(const GtmIndex &ix, const StreamHead &h, int64_t tileset_tiles, int pal_count, tm_gtm_info *o) {
  memset(o, 0, sizeof(*o));
  o->width = ix.width; o->height = ix.height; o->frames = ix.frames; o->keyframes = (int32_t)ix.kf.size();
  o->encoder_version = ix.version; o->avg_bytes_per_s = ix.avg; o->kf_max_bytes_per_s = ix.kf_max;
  o->tm_w = h.tm_w; o->tm_h = h.tm_h; o->tile_count = (int32_t)h.tile_count; o->tileset_tiles = (int32_t)tileset_tiles;
  o->pal_size = h.pal_size; o->pal_count = pal_count;
  o->fps = h.frame_ns ? gtm_fps(h.frame_ns) : 0.0;
  return TM_OK;
}

int probe_gtm(const char *path, int *width, int *height, double *fps, int *frames) {
  FdCloser file{-1};
  GtmIndex ix;
  StreamHead head;
  KfRecords first;
  TM_TRY(open_stream_head(path, &file.fd, &ix, &head, &first));
  *width = head.tm_w * 8; *height = head.tm_h * 8; *frames = ix.frames;
  *fps = gtm_fps(head.frame_ns);
  return TM_OK;
}

}  // namespace tmx

using namespace tmx;

extern "C" {

int tm_player_probe_host(const char *path, tm_gtm_info *info, int32_t *kf, int cap_kf, int *nkf) {
  TM_CHECK(path, TM_E_INVAL, "null argument");
  const int fd = open(path, O_RDONLY);
  TM_CHECK(fd >= 0, TM_E_IO, "cannot open %s", path);
  FdCloser closer{fd};
  GtmIndex ix;
  TM_TRY(read_index(fd, path, &ix));
  if (info) fill_info(ix, StreamHead(), 0, 0, info);
  if (nkf) *nkf = (int)ix.kf.size();
  if (kf)
    for (int k = 0; k < std::min(cap_kf, (int)ix.kf.size()); k++) {
      kf[4 * k] = ix.kf[(size_t)k].frame; kf[4 * k + 1] = (int32_t)ix.kf[(size_t)k].raw; kf[4 * k + 2] = (int32_t)ix.kf[(size_t)k].comp; kf[4 * k + 3] = (int32_t)ix.kf[(size_t)k].ms;
    }
  return TM_OK;
}

int tm_player_parse_host(const uint8_t *raw, size_t n, int tm_w, int tm_h, int64_t tile_count, uint64_t *records, int cap_frames, uint8_t *intra, int64_t cap_intra,
                         int64_t *intra_first, int *frames, int64_t *nintra) {
  TM_CHECK((raw || n == 0) && frames && nintra, TM_E_INVAL, "null argument");
  TM_CHECK(tm_w >= 0 && tm_h >= 0 && tm_w <= 65535 && tm_h <= 65535 && tile_count >= 0, TM_E_INVAL, "bad dimensions %d x %d", tm_w, tm_h);
  TM_CHECK(!records || (tm_w > 0 && tm_h > 0), TM_E_INVAL, "records are sized by tm_w and tm_h: pass them");
  TM_CHECK((int64_t)tm_w * tm_h <= MAX_ITEMS, TM_E_INVAL, "%d x %d tiles: more than %lld items a frame", tm_w, tm_h, (long long)MAX_ITEMS);
  StreamHead head;
  if (tm_w > 0 && tm_h > 0) { head.tm_w = tm_w; head.tm_h = tm_h; head.tile_count = tile_count; head.frame_ns = 1; head.have_dims = true; }
  KfRecords kf;
  TM_TRY(parse_keyframe(raw, n, "key frame", &head, true, true, 0x7fffffff, &kf));
  *frames = kf.nframes;
  *nintra = (int64_t)(kf.intra.size() / 64);
  TM_CHECK((!records && !intra && !intra_first) || (kf.nframes <= cap_frames && *nintra <= cap_intra), TM_E_INVAL, "%d frames and %lld intra tiles: capacities %d and %lld",
           kf.nframes, (long long)*nintra, cap_frames, (long long)cap_intra);
  if (records) memcpy(records, kf.recs.data(), (size_t)kf.nframes * head.tm_w * head.tm_h * sizeof(PlayRec));
  if (intra) memcpy(intra, kf.intra.data(), (size_t)*nintra * 64);
  if (intra_first) memcpy(intra_first, kf.intra_first.data(), ((size_t)kf.nframes + 1) * sizeof(int64_t));
  return TM_OK;
}

}  // extern "C"
