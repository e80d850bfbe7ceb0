// tm_jpeg_in.hip -- the JPEG reader on the device.  The rule is tm_jpeg.h's; the host twin (tm_jpeg_decode_host) runs
// the same text on one lane.
//
//   host      parse_jpeg walks a file's markers (what it accepts and refuses: tm_jpeg.h, include/tilemotion.h) and leaves a descriptor: the
//             quantisers and code tables, the geometry, and the entropy segments as spans of the file, cut at every RSTn.
//   decode    k_jpeg_decode, one workgroup of one wave per picture, every picture of a batch in one launch.  The tables are copied into
//             LDS and the look-ups built there by the whole wave; then every lane takes a segment (in rounds of 64): a 64-bit bit buffer
//             in registers, the block's coefficients in the lane's own LDS slot (128 bytes, slots 132 apart so that the lanes' words fall
//             into different banks), the inverse DCT out of that slot in registers, eight 8-byte stores into the plane.  No coefficient
//             goes to HBM.  The input is not staged: a lane's refill fetches its segment's bytes one by one from HBM, every lane at an
//             address of its own, so the loads do not coalesce (not tuned: DESIGN.md section 39.4).  A file without restart markers is one lane's work, as a zlib stream is one wave's in k_inflate: a batch of
//             hundreds of files is what fills the device.
//   colour    none here: the planes go through k_yuv_to_rgb32 (tm_yuv_in.hip) as a lent YUV clip's do.
//
// Every loop is bounded by a segment's bytes, its MCUs or the picture's segments (tm_jpeg.h: decode_segment); plain launches, nothing
// waits on another workgroup.
#include "tm_input.h"
#include "tm_jpeg.h"

namespace tmx {
namespace jpg {
namespace {

static_assert(sizeof(Frame) % 8 == 0 && sizeof(TableSet) % 8 == 0 && sizeof(TableSet) % 4 == 0, "the descriptor's parts follow one another on 8 bytes");

// ---- the host IO: one lane
struct HostIO {
  uint16_t fast_[kCodeTables << kFastBits];
  alignas(8) int16_t slot_[64];
  uint32_t first = kNoRefusal;
  int st = kOk;
  uint32_t lane() const { return 0; }
  uint32_t lanes() const { return 1; }
  void sync() {}
  uint16_t *fast() { return fast_; }
  int16_t *slot() { return slot_; }
  void refuse(uint32_t i) { if (i < first) first = i; }
  uint32_t refusal() const { return first; }
  void set_status(int rc) { st = rc; }
  int status() const { return st; }
};

// ---- the device IO: one wave, a lane per segment
struct WaveLds {
  Frame frame;  // (in LDS, not in registers: its arrays are indexed by the component; so are the planes' pointers)
  uint8_t *planes[3];
  TableSet ts;
  uint16_t fast[kCodeTables << kFastBits];
  int16_t slots[64 * kSlotHalves];
  uint32_t first;
  int32_t st;
};
struct WaveIO {
  WaveLds &m;
  __device__ uint32_t lane() const { return threadIdx.x; }
  __device__ uint32_t lanes() const { return 64; }
  __device__ void sync() { __syncthreads(); }  // (the workgroup is this wave)
  __device__ uint16_t *fast() { return m.fast; }
  __device__ int16_t *slot() { return m.slots + threadIdx.x * kSlotHalves; }
  __device__ void refuse(uint32_t i) { atomicMin(&m.first, i); }
  __device__ uint32_t refusal() const { return m.first; }
  __device__ void set_status(int rc) { m.st = rc; }
  __device__ int status() const { return m.st; }
};

// One wave per picture.  A frame whose segments or planes do not lie inside what the launch was given is refused untouched.
__global__ __launch_bounds__(64) void k_jpeg_decode(const uint8_t *__restrict__ blob, uint64_t blob_bytes, const Frame *__restrict__ frames,
                                                    const TableSet *__restrict__ tables, const Seg *__restrict__ segs, uint32_t nsegs, uint8_t *y, uint8_t *u, uint8_t *v,
                                                    uint64_t y_bytes, uint64_t u_bytes, uint64_t v_bytes, int32_t *__restrict__ status) {
  __shared__ __align__(16) WaveLds lds;
  const uint32_t p = blockIdx.x, lane = threadIdx.x;
  {
    const uint32_t *from = reinterpret_cast<const uint32_t *>(frames + p);
    uint32_t *to = reinterpret_cast<uint32_t *>(&lds.frame);
    for (uint32_t i = lane; i < sizeof(Frame) / 4; i += 64) to[i] = from[i];
  }
  __syncthreads();
  const Frame &f = lds.frame;
  const uint64_t plane_bytes[3] = {y_bytes, u_bytes, v_bytes};
  if (!frame_ok(f, nsegs, plane_bytes)) {  // (the same in every lane)
    if (lane == 0) status[p] = kBadDesc;
    return;
  }
  const uint32_t *from = reinterpret_cast<const uint32_t *>(tables + p);
  uint32_t *to = reinterpret_cast<uint32_t *>(&lds.ts);
  for (uint32_t i = lane; i < sizeof(TableSet) / 4; i += 64) to[i] = from[i];
  if (lane == 0) { lds.first = kNoRefusal; lds.st = kOk; lds.planes[0] = y; lds.planes[1] = u; lds.planes[2] = v; }
  __syncthreads();
  WaveIO io{lds};
  const int rc = decode_frame(io, f, lds.ts, segs, blob, blob_bytes, lds.planes);
  if (lane == 0) status[p] = rc;
}

uint32_t be16(const uint8_t *p) { return (uint32_t)p[0] << 8 | p[1]; }

// the code tables of T.81 Annex K.3 (tables K.3 .. K.6), for a file that carries none
const uint8_t kStdDcLumaCounts[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kStdDcChromaCounts[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kStdAcLumaCounts[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kStdAcChromaCounts[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kStdAcLuma[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kStdAcChroma[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
    0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
void standard_tables(TableSet *ts) {
  memset(ts->count, 0, sizeof(ts->count));
  memset(ts->symbol, 0, sizeof(ts->symbol));
  memcpy(ts->count[0], kStdDcLumaCounts, 16); memcpy(ts->count[1], kStdDcChromaCounts, 16);
  memcpy(ts->count[4], kStdAcLumaCounts, 16); memcpy(ts->count[5], kStdAcChromaCounts, 16);
  for (int i = 0; i < 12; i++) ts->symbol[0][i] = ts->symbol[1][i] = (uint8_t)i;
  memcpy(ts->symbol[4], kStdAcLuma, 162); memcpy(ts->symbol[5], kStdAcChroma, 162);
}

const char *marker_name(uint32_t m, char buf[16]) {
  if (m >= 0xc0 && m <= 0xcf && m != 0xc4 && m != 0xc8 && m != 0xcc) snprintf(buf, 16, "SOF%u", m - 0xc0);
  else if (m >= 0xe0 && m <= 0xef) snprintf(buf, 16, "APP%u", m - 0xe0);
  else if (m >= 0xd0 && m <= 0xd7) snprintf(buf, 16, "RST%u", m - 0xd0);
  else snprintf(buf, 16, "%s", m == 0xc4 ? "DHT" : m == 0xdb ? "DQT" : m == 0xdd ? "DRI" : m == 0xda ? "SOS" : m == 0xfe ? "COM" : m == 0xdc ? "DNL" : m == 0xd9 ? "EOI" :
                                 m == 0xd8 ? "SOI" : m == 0xcc ? "DAC" : "marker");
  return buf;
}

int check_files(const char *who, const void *const *files, const size_t *sizes, int nfiles, int w, int h, const void *y, const int64_t *strides, const int32_t *status) {
  TM_CHECK(files && sizes && y && strides && status && nfiles >= 0, TM_E_INVAL, "%s: null argument", who);
  TM_CHECK(w >= 1 && h >= 1 && w <= 65535 && h <= 65535, TM_E_INVAL, "%s: bad size %dx%d", who, w, h);
  for (int i = 0; i < 6; i++) TM_CHECK(strides[i] >= 0 && strides[i] < ((int64_t)1 << 31), TM_E_INVAL, "%s: stride %d is %lld (0 .. 2^31 - 1)", who, i, (long long)strides[i]);
  for (int i = 0; i < nfiles; i++) TM_CHECK(files[i], TM_E_INVAL, "%s: file %d is null", who, i);
  return TM_OK;
}

// the files of one of the two entry points walked and laid out: file i's planes at frame stride i of the caller's, at the file's own size
int plan_files(const char *who, const void *const *files, const size_t *sizes, int nfiles, int w, int h, const void *u, const void *v, const int64_t *strides,
               std::vector<JpegInfo> *infos, std::vector<PlaneLayout> *layouts, JpegBatch *batch, std::vector<uint64_t> *where, uint64_t plane_bytes[3]) {
  infos->resize((size_t)nfiles);
  layouts->resize((size_t)nfiles);
  where->resize((size_t)nfiles);
  uint64_t at = 0;
  plane_bytes[0] = plane_bytes[1] = plane_bytes[2] = 0;
  for (int i = 0; i < nfiles; i++) {
    char name[32];
    snprintf(name, sizeof(name), "file %d", i);
    JpegInfo &info = (*infos)[(size_t)i];
    TM_TRY(parse_jpeg((const uint8_t *)files[i], sizes[i], name, &info));
    TM_CHECK(info.w <= w && info.h <= h, TM_E_INVAL, "%s: %s is %dx%d, the planes hold %dx%d", who, name, info.w, info.h, w, h);
    TM_CHECK(info.ncomp == 1 || (u && v), TM_E_INVAL, "%s: %s has chroma, but u or v is null", who, name);
    PlaneLayout pl;
    for (int c = 0; c < info.ncomp; c++) {
      int pw, ph;
      info.plane_size(c, &pw, &ph);
      const int64_t row = strides[2 * c], frame = strides[2 * c + 1];
      TM_CHECK(row >= pw && (nfiles == 1 || frame >= row * ph), TM_E_INVAL, "%s: %s: the strides of plane %d are shorter than its %dx%d samples", who, name, c, pw, ph);
      pl.off[c] = (uint64_t)frame * (uint64_t)i; pl.stride[c] = (uint32_t)row; pl.w[c] = (uint32_t)pw; pl.h[c] = (uint32_t)ph;
      plane_bytes[c] = std::max(plane_bytes[c], pl.off[c] + (uint64_t)(ph - 1) * (uint64_t)row + (uint64_t)pw);
    }
    (*where)[(size_t)i] = at;
    (*layouts)[(size_t)i] = pl;
    if (batch) batch->add(info, at, pl);
    at += (sizes[i] + 15) & ~(size_t)15;
  }
  TM_CHECK(!batch || at + batch->desc_bytes() < ((uint64_t)1 << 32), TM_E_UNSUPPORTED, "%s: a batch of %llu bytes (below 4 GiB)", who, (unsigned long long)at);
  return TM_OK;
}

}  // namespace

void JpegInfo::plane_size(int c, int *pw, int *ph) const {
  const bool sub = c > 0 && ncomp == 3;
  *pw = sub ? (w + hs - 1) / hs : w;
  *ph = sub ? (h + vs - 1) / vs : h;
}
void JpegInfo::mcus(uint32_t *across, uint32_t *down) const {
  const int bw = ncomp == 1 ? 8 : 8 * hs, bh = ncomp == 1 ? 8 : 8 * vs;
  *across = (uint32_t)((w + bw - 1) / bw);
  *down = (uint32_t)((h + bh - 1) / bh);
}
int JpegInfo::layout() const { return ncomp == 1 ? TM_CHROMA_MONO : hs == 1 ? TM_CHROMA_444 : vs == 1 ? CHROMA_422_CENTRED : TM_CHROMA_420JPEG; }

// ---- the container walk
int parse_jpeg(const uint8_t *file, size_t n, const char *name, JpegInfo *info) {
  TM_CHECK(n >= 2 && file[0] == 0xff && file[1] == 0xd8, TM_E_IO, "%s: no SOI marker: not a JPEG file", name);
  TM_CHECK(n < ((size_t)1 << 32), TM_E_UNSUPPORTED, "%s: a file of %zu bytes (below 4 GiB)", name, n);
  JpegInfo &o = *info;
  o.w = o.h = o.ncomp = 0; o.hs = o.vs = 1; o.sof = -1; o.ri = 0; o.status0 = kOk;
  o.segs.clear();
  memset(&o.ts, 0, sizeof(o.ts));
  bool have_q[4] = {false, false, false, false}, have_code[kCodeTables] = {false, false, false, false, false, false, false, false}, any_dht = false;
  uint8_t comp_id[4] = {0, 0, 0, 0};
  int adobe_transform = -1;
  char mn[16];
  size_t pos = 2;
  for (;;) {
    TM_CHECK(pos < n, TM_E_IO, "%s: the file ends before a scan (no SOS)", name);
    TM_CHECK(file[pos] == 0xff, TM_E_IO, "%s: byte %zu is 0x%02x where a marker is expected", name, pos, file[pos]);
    while (pos < n && file[pos] == 0xff) pos++;  // (fill bytes)
    TM_CHECK(pos < n, TM_E_IO, "%s: the file ends before a scan (no SOS)", name);
    const uint32_t m = file[pos++];
    TM_CHECK(m != 0xd9, TM_E_IO, "%s: EOI before any scan", name);
    TM_CHECK(m != 0xd8 && m != 0x00 && !(m >= 0xd0 && m <= 0xd7), TM_E_IO, "%s: a %s marker (0xff%02x) outside a scan", name, marker_name(m, mn), m);
    if (m == 0x01) continue;  // TEM: no length
    TM_CHECK(pos + 2 <= n, TM_E_IO, "%s: the %s segment runs past the file", name, marker_name(m, mn));
    const size_t len = be16(file + pos);
    TM_CHECK(len >= 2 && len <= n - pos, TM_E_IO, "%s: the %s segment runs past the file", name, marker_name(m, mn));
    const uint8_t *d = file + pos + 2;
    const size_t dn = len - 2;
    pos += len;
    if (m == 0xc0 || m == 0xc1) {
      TM_CHECK(o.sof < 0, TM_E_UNSUPPORTED, "%s: a second frame header (%s)", name, marker_name(m, mn));
      TM_CHECK(dn >= 6, TM_E_IO, "%s: the %s segment is too short", name, marker_name(m, mn));
      TM_CHECK(d[0] == 8, TM_E_UNSUPPORTED, "%s: precision %d in %s (8 bits only)", name, d[0], marker_name(m, mn));
      o.h = (int)be16(d + 1); o.w = (int)be16(d + 3);
      TM_CHECK(o.h != 0, TM_E_UNSUPPORTED, "%s: height 0 in %s (the height is to come in a DNL segment)", name, marker_name(m, mn));
      TM_CHECK(o.w != 0, TM_E_IO, "%s: width 0 in %s", name, marker_name(m, mn));
      const int nc = d[5];
      TM_CHECK(nc != 2 && nc != 4, TM_E_UNSUPPORTED, "%s: %d components in %s (1 or 3)", name, nc, marker_name(m, mn));
      TM_CHECK((nc == 1 || nc == 3) && dn == 6 + 3 * (size_t)nc, TM_E_IO, "%s: %d components in a %s segment of %zu bytes", name, nc, marker_name(m, mn), len);
      int hv[3][2];
      for (int c = 0; c < nc; c++) {
        comp_id[c] = d[6 + 3 * c];
        hv[c][0] = d[7 + 3 * c] >> 4; hv[c][1] = d[7 + 3 * c] & 15;
        TM_CHECK(hv[c][0] >= 1 && hv[c][0] <= 4 && hv[c][1] >= 1 && hv[c][1] <= 4, TM_E_IO, "%s: sampling factors %dx%d of component %d", name, hv[c][0], hv[c][1], c);
        TM_CHECK(d[8 + 3 * c] <= 3, TM_E_IO, "%s: component %d names quantiser %d", name, c, d[8 + 3 * c]);
        o.tq[c] = d[8 + 3 * c];
      }
      if (nc == 3) {
        const bool ok = hv[1][0] == 1 && hv[1][1] == 1 && hv[2][0] == 1 && hv[2][1] == 1 && (hv[0][0] == 1 || hv[0][0] == 2) && (hv[0][1] == 1 || hv[0][1] == 2) &&
                        !(hv[0][0] == 1 && hv[0][1] == 2);
        TM_CHECK(ok, TM_E_UNSUPPORTED, "%s: sampling %dx%d,%dx%d,%dx%d (4:4:4, 4:2:2 and 4:2:0 only)", name, hv[0][0], hv[0][1], hv[1][0], hv[1][1], hv[2][0], hv[2][1]);
        o.hs = hv[0][0]; o.vs = hv[0][1];
      }
      o.ncomp = nc; o.sof = (int)m - 0xc0;
    } else if (m >= 0xc0 && m <= 0xcf && m != 0xc4) {
      if (m == 0xc2) { set_error("%s: SOF2: progressive files are not read", name); return TM_E_UNSUPPORTED; }
      set_error("%s: %s: lossless, differential and arithmetic-coded files are not read", name, m == 0xcc ? "DAC" : m == 0xc8 ? "JPG" : marker_name(m, mn));
      return TM_E_UNSUPPORTED;
    } else if (m == 0xdb) {
      for (size_t at = 0; at < dn;) {
        const int pq = d[at] >> 4, tq = d[at] & 15;
        TM_CHECK(pq <= 1 && tq <= 3, TM_E_IO, "%s: DQT: precision %d, table %d", name, pq, tq);
        const size_t need = 1 + (size_t)64 * (pq + 1);
        TM_CHECK(need <= dn - at, TM_E_IO, "%s: DQT: table %d runs past its segment", name, tq);
        for (uint32_t k = 0; k < 64; k++) o.ts.q[tq][zigzag(k)] = (uint16_t)(pq ? be16(d + at + 1 + 2 * k) : d[at + 1 + k]);
        have_q[tq] = true;
        at += need;
      }
    } else if (m == 0xc4) {
      for (size_t at = 0; at < dn;) {
        const int tc = d[at] >> 4, th = d[at] & 15;
        TM_CHECK(tc <= 1 && th <= 3, TM_E_IO, "%s: DHT: class %d, table %d", name, tc, th);
        TM_CHECK(17 <= dn - at, TM_E_IO, "%s: DHT: table %d/%d runs past its segment", name, tc, th);
        int total = 0, left = 1;
        for (int l = 0; l < 16; l++) {
          total += d[at + 1 + l];
          left = (left << 1) - d[at + 1 + l];
          TM_CHECK(left >= 0, TM_E_IO, "%s: DHT: the counts of table %d/%d over-subscribe the code space at length %d", name, tc, th, l + 1);
        }
        TM_CHECK(total <= 256, TM_E_IO, "%s: DHT: table %d/%d names %d symbols (256 at most)", name, tc, th, total);
        TM_CHECK((size_t)total <= dn - at - 17, TM_E_IO, "%s: DHT: table %d/%d runs past its segment", name, tc, th);
        const int t = tc << 2 | th;
        memcpy(o.ts.count[t], d + at + 1, 16);
        memset(o.ts.symbol[t], 0, 256);
        memcpy(o.ts.symbol[t], d + at + 17, (size_t)total);
        have_code[t] = true; any_dht = true;
        at += 17 + (size_t)total;
      }
    } else if (m == 0xdd) {
      TM_CHECK(dn == 2, TM_E_IO, "%s: a DRI segment of %zu bytes", name, len);
      o.ri = be16(d);
    } else if (m == 0xdc) {
      set_error("%s: DNL: a height given behind the scan is not read", name);
      return TM_E_UNSUPPORTED;
    } else if (m == 0xde || m == 0xdf) {
      set_error("%s: hierarchical files (marker 0xff%02x) are not read", name, m);
      return TM_E_UNSUPPORTED;
    } else if (m == 0xee) {
      if (dn >= 12 && !memcmp(d, "Adobe", 5)) adobe_transform = d[11];
    } else if (m == 0xda) {
      TM_CHECK(o.sof >= 0, TM_E_IO, "%s: SOS before a frame header", name);
      TM_CHECK(dn >= 1, TM_E_IO, "%s: the SOS segment is too short", name);
      const int ns = d[0];
      TM_CHECK(ns >= 1 && ns <= 4 && dn == 4 + 2 * (size_t)ns, TM_E_IO, "%s: SOS: %d components in a segment of %zu bytes", name, ns, len);
      for (int j = 0; j < ns; j++) {
        int c = 0;
        while (c < o.ncomp && comp_id[c] != d[1 + 2 * j]) c++;
        TM_CHECK(c < o.ncomp, TM_E_IO, "%s: SOS names component %d, which the frame does not have", name, d[1 + 2 * j]);
      }
      TM_CHECK(ns == o.ncomp, TM_E_UNSUPPORTED, "%s: a scan of %d of the %d components: more than one scan", name, ns, o.ncomp);
      for (int j = 0; j < ns; j++) {
        TM_CHECK(comp_id[j] == d[1 + 2 * j], TM_E_UNSUPPORTED, "%s: SOS lists the components in another order than the frame", name);
        o.td[j] = d[2 + 2 * j] >> 4; o.ta[j] = d[2 + 2 * j] & 15;
        TM_CHECK(o.td[j] <= 3 && o.ta[j] <= 3, TM_E_IO, "%s: SOS: component %d names tables %d/%d", name, j, o.td[j], o.ta[j]);
      }
      const uint8_t *tail = d + 1 + 2 * ns;
      TM_CHECK(tail[0] == 0 && tail[1] == 63 && tail[2] == 0, TM_E_UNSUPPORTED, "%s: SOS: Ss %d, Se %d, Ah/Al 0x%02x (a sequential scan has 0, 63, 0)", name, tail[0], tail[1], tail[2]);
      TM_CHECK(!(o.ncomp == 3 && adobe_transform == 0), TM_E_UNSUPPORTED, "%s: APP14 (Adobe) transform 0: the three components are RGB", name);
      if (!any_dht) {
        standard_tables(&o.ts);
        have_code[0] = have_code[1] = have_code[4] = have_code[5] = true;
      }
      for (int j = 0; j < ns; j++) {
        TM_CHECK(have_q[o.tq[j]], TM_E_IO, "%s: component %d names quantiser %d, which no DQT defines", name, j, o.tq[j]);
        TM_CHECK(have_code[o.td[j]], TM_E_IO, "%s: SOS: component %d names DC table %d, which no DHT defines", name, j, o.td[j]);
        TM_CHECK(have_code[4 + o.ta[j]], TM_E_IO, "%s: SOS: component %d names AC table %d, which no DHT defines", name, j, o.ta[j]);
      }
      break;
    }
    // APPn, COM and whatever else carries a length: skipped
  }
  // the scan: cut at every RSTn; FF 00 and fill bytes are no cuts; any other marker ends it
  uint32_t mcx, mcy;
  o.mcus(&mcx, &mcy);
  const uint64_t total = (uint64_t)mcx * mcy;
  size_t start = pos, p = pos;
  uint32_t end_marker = 0;
  bool in_order = true;
  while (p < n) {
    if (file[p] != 0xff) { p++; continue; }
    if (p + 1 < n && file[p + 1] == 0x00) { p += 2; continue; }
    size_t q = p;
    while (q < n && file[q] == 0xff) q++;
    if (q >= n) { p = n; break; }  // (a cut file: the data runs to its end)
    const uint32_t m = file[q];
    if (m == 0x00) { p = q + 1; continue; }  // FF .. FF 00: fill bytes before a stuffed FF -- the last FF is data
    o.segs.push_back(Seg{(uint32_t)start, (uint32_t)(p - start)});
    if (m >= 0xd0 && m <= 0xd7) {
      if (m - 0xd0 != ((o.segs.size() - 1) & 7u)) in_order = false;
      start = p = q + 1;
      continue;
    }
    end_marker = m;
    p = q + 1;
    start = (size_t)-1;
    break;
  }
  if (start != (size_t)-1) o.segs.push_back(Seg{(uint32_t)start, (uint32_t)(n - start)});  // no marker behind the data
  // what follows the scan, up to EOI
  for (uint32_t m = end_marker; m && m != 0xd9;) {
    TM_CHECK(m != 0xda, TM_E_UNSUPPORTED, "%s: a second SOS: more than one scan", name);
    TM_CHECK(m != 0xdc, TM_E_UNSUPPORTED, "%s: DNL: a height given behind the scan is not read", name);
    TM_CHECK(p + 2 <= n, TM_E_IO, "%s: the %s segment behind the scan runs past the file", name, marker_name(m, mn));
    const size_t len = be16(file + p);
    TM_CHECK(len >= 2 && len <= n - p, TM_E_IO, "%s: the %s segment behind the scan runs past the file", name, marker_name(m, mn));
    p += len;
    while (p < n && file[p] == 0xff) p++;
    if (p >= n) break;
    m = file[p++];
  }
  const uint32_t ri = o.ri ? o.ri : (uint32_t)std::min<uint64_t>(total, 0xffffffffu);
  const uint64_t want = (total + ri - 1) / ri;
  o.nsegs = (uint32_t)std::min<size_t>(o.segs.size(), 0x7fffffffu);
  if (!in_order || o.segs.size() != want) {  // (such a file is not decoded: its list, which may be as long as the file, is dropped)
    o.status0 = kBadRestart;
    o.segs.clear();
  }
  return TM_OK;
}

// a refused file's status as Load's error
int jpeg_status_error(int status, const char *name) {
  if (status == kOk) return TM_OK;
  const char *what = status == kTruncated ? "the entropy data ends inside a symbol (TM_JPG_TRUNCATED)" : status == kBadCode ? "bits that are no code (TM_JPG_BAD_CODE)" :
                     status == kBadRun ? "a zero run past the 64th coefficient (TM_JPG_BAD_RUN)" : status == kBadMagnitude ? "a coefficient category out of range (TM_JPG_BAD_MAGNITUDE)" :
                     status == kBadRestart ? "a restart marker is missing or out of sequence (TM_JPG_BAD_RESTART)" : "the descriptor was refused (TM_JPG_BAD_DESC)";
  set_error("%s: %s", name, what);
  return TM_E_INVAL;
}

void JpegBatch::clear() { frames.clear(); tables.clear(); segs.clear(); }
void JpegBatch::add(const JpegInfo &info, uint64_t at, const PlaneLayout &pl) {
  Frame f;
  memset(&f, 0, sizeof(f));
  for (int c = 0; c < info.ncomp; c++) {
    f.plane_off[c] = pl.off[c]; f.plane_stride[c] = pl.stride[c]; f.plane_w[c] = pl.w[c]; f.plane_h[c] = pl.h[c];
    f.tq[c] = info.tq[c]; f.td[c] = info.td[c]; f.ta[c] = info.ta[c];
  }
  uint32_t mcx, mcy;
  info.mcus(&mcx, &mcy);
  f.seg_first = (uint32_t)segs.size(); f.seg_count = (uint32_t)info.segs.size();
  f.mcus_x = mcx; f.mcus_total = mcx * mcy;
  f.ri = info.ri ? info.ri : f.mcus_total;
  f.ncomp = (uint32_t)info.ncomp; f.hs = (uint32_t)info.hs; f.vs = (uint32_t)info.vs;
  f.status0 = info.status0;
  for (const Seg &sg : info.segs) segs.push_back(Seg{(uint32_t)(at + sg.off), sg.len});
  frames.push_back(f);
  tables.push_back(info.ts);
}
size_t JpegBatch::desc_bytes() const { return frames.size() * (sizeof(Frame) + sizeof(TableSet)) + segs.size() * sizeof(Seg) + 16; }
// frames | table sets | segments
size_t JpegBatch::write_desc(uint8_t *to) const {
  size_t at = 0;
  memcpy(to + at, frames.data(), frames.size() * sizeof(Frame)); at += frames.size() * sizeof(Frame);
  memcpy(to + at, tables.data(), tables.size() * sizeof(TableSet)); at += tables.size() * sizeof(TableSet);
  if (!segs.empty()) memcpy(to + at, segs.data(), segs.size() * sizeof(Seg));
  at += segs.size() * sizeof(Seg);
  return at;
}

// the kernel on a batch whose files and descriptor (write_desc at desc_off, a multiple of 8) lie in the device blob
int jpeg_batch_launch(const JpegBatch &b, const uint8_t *dev_blob, size_t blob_bytes, size_t desc_off, uint8_t *y, uint8_t *u, uint8_t *v, const uint64_t plane_bytes[3],
                      int32_t *dev_status, void *hip_stream) {
  const int n = (int)b.frames.size();
  if (!n) return TM_OK;
  const uint8_t *d = dev_blob + desc_off;
  const Frame *frames = reinterpret_cast<const Frame *>(d);
  const TableSet *tables = reinterpret_cast<const TableSet *>(d + (size_t)n * sizeof(Frame));
  const Seg *segs = reinterpret_cast<const Seg *>(d + (size_t)n * (sizeof(Frame) + sizeof(TableSet)));
  hipLaunchKernelGGL(k_jpeg_decode, dim3((unsigned)n), dim3(64), 0, (hipStream_t)hip_stream, dev_blob, (uint64_t)blob_bytes, frames, tables, segs, (uint32_t)b.segs.size(), y, u,
                     v, plane_bytes[0], plane_bytes[1], plane_bytes[2], dev_status);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

// one walked file on the host: the rule on one lane
int jpeg_decode_one_host(const JpegInfo &info, const uint8_t *file, size_t n, const PlaneLayout &pl, uint8_t *const planes[3]) {
  JpegBatch one;
  one.add(info, 0, pl);
  std::vector<HostIO> io(1);  // (its tables are 8 KB: not on a reader thread's stack)
  return decode_frame(io[0], one.frames[0], one.tables[0], one.segs.data(), file, (uint64_t)n, planes);
}

}  // namespace jpg
}  // namespace tmx

using namespace tmx;

extern "C" {

int tm_probe_jpeg_host(const void *file, size_t size, tm_jpeg_info *out) {
  TM_CHECK(file && out, TM_E_INVAL, "tm_probe_jpeg_host: null argument");
  jpg::JpegInfo info;
  TM_TRY(jpg::parse_jpeg((const uint8_t *)file, size, "file", &info));
  out->width = info.w; out->height = info.h; out->components = info.ncomp; out->h_samp = info.hs; out->v_samp = info.vs;
  out->restart_interval = (int32_t)info.ri; out->segments = (int32_t)info.nsegs; out->sof = info.sof;
  out->chroma = info.layout() == CHROMA_422_CENTRED ? (int)TM_CHROMA_422 : info.layout();
  out->status = info.status0;
  return TM_OK;
}

int tm_jpeg_decode_host(const void *const *files, const size_t *sizes, int nfiles, int w, int h, uint8_t *y, uint8_t *u, uint8_t *v, const int64_t *strides, int32_t *status) {
  TM_TRY(jpg::check_files("tm_jpeg_decode_host", files, sizes, nfiles, w, h, y, strides, status));
  std::vector<jpg::JpegInfo> infos;
  std::vector<jpg::PlaneLayout> layouts;
  std::vector<uint64_t> where;
  uint64_t plane_bytes[3];
  TM_TRY(jpg::plan_files("tm_jpeg_decode_host", files, sizes, nfiles, w, h, u, v, strides, &infos, &layouts, nullptr, &where, plane_bytes));
  uint8_t *const planes[3] = {y, u, v};
  for (int i = 0; i < nfiles; i++) status[i] = jpg::jpeg_decode_one_host(infos[(size_t)i], (const uint8_t *)files[i], sizes[i], layouts[(size_t)i], planes);
  return TM_OK;
}

int tm_stage_jpeg_decode(const void *const *files, const size_t *sizes, int nfiles, int w, int h, uint8_t *dev_y, uint8_t *dev_u, uint8_t *dev_v, const int64_t *strides,
                         int32_t *status, void *stream) {
  TM_TRY(jpg::check_files("tm_stage_jpeg_decode", files, sizes, nfiles, w, h, dev_y, strides, status));
  std::vector<jpg::JpegInfo> infos;
  std::vector<jpg::PlaneLayout> layouts;
  std::vector<uint64_t> where;
  jpg::JpegBatch batch;
  uint64_t plane_bytes[3];
  TM_TRY(jpg::plan_files("tm_stage_jpeg_decode", files, sizes, nfiles, w, h, dev_u, dev_v, strides, &infos, &layouts, &batch, &where, plane_bytes));
  TM_TRY(require_device());
  if (!nfiles) return TM_OK;
  hipStream_t hs = (hipStream_t)stream;
  size_t at = 0;
  for (int i = 0; i < nfiles; i++) at = (size_t)where[(size_t)i] + ((sizes[i] + 15) & ~(size_t)15);
  std::vector<uint8_t> blob(at + batch.desc_bytes());
  for (int i = 0; i < nfiles; i++) memcpy(blob.data() + where[(size_t)i], files[i], sizes[i]);
  const size_t used = at + batch.write_desc(blob.data() + at);
  DevBuf d_blob, d_status;
  TM_TRY(d_blob.alloc(used)); TM_TRY(d_status.alloc((size_t)nfiles * 4));
  TM_HIP(hipMemcpyAsync(d_blob.p, blob.data(), used, hipMemcpyHostToDevice, hs));
  TM_TRY(jpg::jpeg_batch_launch(batch, d_blob.as<uint8_t>(), used, at, dev_y, dev_u, dev_v, plane_bytes, d_status.as<int32_t>(), hs));
  TM_HIP(hipMemcpyAsync(status, d_status.p, (size_t)nfiles * 4, hipMemcpyDeviceToHost, hs));
  TM_HIP(hipStreamSynchronize(hs));
  return TM_OK;
}

}  // extern "C"
