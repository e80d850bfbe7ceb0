// tm_resample.hip -- the Lanczos-3 resampling tables (host only): the one place the rule of DESIGN.md section 17 is stated.  Its two users are
// the kernel that reads YUV planes on the way in (tm_yuv_in.hip) and the kernel that scales RGB32 frames on the way out (tm_scale.hip):
//   r = n / m;  f = max(1, r / s);  u_j = ((j + 0.5) r - 0.5 - o) / s;  taps ceil(u_j - 3f) .. floor(u_j + 3f) inside the plane
//   c_k = RoundHalfEven(16384 w_k / sum w), the remainder to the tap of largest w;  h = (sum c p + 64) >> 7;  v = clamp((sum c h + 2^20) >> 21)
// for a plane whose samples sit at luma positions s k + o (s = 2 for subsampled chroma, o = 0.5 where it is centred).
#include <cmath>

#include "tm_internal.h"

namespace tmx {

static double lanczos3(double t) {
  t = std::fabs(t);
  if (t >= 3.0) return 0.0;
  if (t == 0.0) return 1.0;
  const double x = M_PI * t;
  return (std::sin(x) / x) * (std::sin(x / 3.0) / (x / 3.0));
}

// one axis: n luma samples in, m samples out, a plane of np samples at luma positions s k + o_halves / 2.  first / count [m], coef [m][64].
int resample_taps(int n, int m, int np, int s, int o_halves, int32_t *first, int32_t *count, int32_t *coef, int64_t *sum_abs_max) {
  TM_CHECK(n > 0 && m > 0 && np > 0 && (s == 1 || s == 2) && (o_halves == 0 || o_halves == 1), TM_E_INVAL, "resample: bad axis %d -> %d (plane %d, step %d)", n, m, np, s);
  const double r = (double)n / (double)m;
  TM_CHECK(r / s <= 8.0, TM_E_UNSUPPORTED, "resample: %d -> %d samples shrinks by more than 8 (more than %d taps)", n, m, TM_RESAMPLE_MAX_TAPS);
  const double f = std::max(1.0, r / s), o = o_halves * 0.5;
  int64_t amax = 0;
  for (int j = 0; j < m; j++) {
    const double x = (j + 0.5) * r - 0.5;
    const double u = (x - o) / s;
    const int k0 = (int)std::max(0.0, std::ceil(u - 3.0 * f)), k1 = (int)std::min((double)(np - 1), std::floor(u + 3.0 * f));
    const int cnt = k1 - k0 + 1;
    TM_CHECK(cnt >= 1 && cnt <= TM_RESAMPLE_MAX_TAPS, TM_E_UNSUPPORTED, "resample: %d taps for sample %d of %d -> %d", cnt, j, n, m);
    double w[TM_RESAMPLE_MAX_TAPS], tot = 0.0;
    for (int k = 0; k < cnt; k++) { w[k] = lanczos3(((double)(k0 + k) - u) / f); tot += w[k]; }
    int32_t *c = coef + (size_t)j * TM_RESAMPLE_MAX_TAPS;
    int64_t sum = 0, sa = 0;
    int best = 0;
    for (int k = 0; k < TM_RESAMPLE_MAX_TAPS; k++) c[k] = 0;
    for (int k = 0; k < cnt; k++) {
      c[k] = (int32_t)std::nearbyint(w[k] / tot * 16384.0);  // (round half to even: the default rounding mode)
      sum += c[k];
      if (w[k] > w[best]) best = k;  // the lowest k on a tie
    }
    c[best] += (int32_t)(16384 - sum);
    for (int k = 0; k < cnt; k++) sa += std::abs(c[k]);
    amax = std::max(amax, sa);
    first[j] = k0;
    count[j] = cnt;
  }
  if (sum_abs_max) *sum_abs_max = amax;
  return TM_OK;
}

int AxisTable::make(int n, int m_out, int np, int s, int o_halves) {
  m = m_out;
  if (m > 0) { first.assign(m, 0); count.assign(m, 0); coef.assign((size_t)m * TM_RESAMPLE_MAX_TAPS, 0); }
  return resample_taps(n, m, np, s, o_halves, first.data(), count.data(), coef.data(), &amax);
}

// the vertical sum fits int32: |h| <= 255 A_h / 128 + 1, |sum| <= that times A_v
int check_resample_sums(const AxisTable &h, const AxisTable &v, int src_w, int src_h, int dst_w, int dst_h) {
  TM_CHECK((255 * h.amax / 128 + 1) * v.amax < (1ll << 31), TM_E_UNSUPPORTED, "resample: the coefficients of %dx%d -> %dx%d overflow the 32-bit sums", src_w, src_h, dst_w,
           dst_h);
  return TM_OK;
}

// A sample's taps start at its first and end at its last coefficient that is not 0 (the sums are the same): at equal size the window still
// spans the six neighbours at whole distances, whose weights sin(k pi) round to 0 -- one tap is left, the sample itself.
// (trimmed windows need no longer be ordered along the axis: the rows a tile reaches are the span of all its samples' windows)
void AxisTable::trim() {
  for (int j = 0; j < m; j++) {
    int32_t *c = &coef[(size_t)j * TM_RESAMPLE_MAX_TAPS];
    int lo = 0, hi = count[j];
    while (hi - lo > 1 && c[hi - 1] == 0) hi--;
    while (hi - lo > 1 && c[lo] == 0) lo++;
    for (int k = 0; k < hi - lo; k++) c[k] = c[lo + k];
    first[j] += lo;
    count[j] = hi - lo;
  }
}

// the source rows the samples of every tile of th output rows reach, as (first row, number of rows) per tile
std::vector<int32_t> AxisTable::tile_spans(int th, int *widest) const {
  std::vector<int32_t> sp;
  for (int y0 = 0; y0 < m; y0 += th) {
    int r0 = INT32_MAX, r1 = 0;
    for (int y = y0; y < std::min(y0 + th, m); y++) { r0 = std::min(r0, first[y]); r1 = std::max(r1, first[y] + count[y]); }
    sp.push_back(r0); sp.push_back(r1 - r0);
    *widest = std::max(*widest, r1 - r0);
  }
  return sp;
}

// the tile height: the largest of 16, 8, 4, 2, 1 for which no tile's vertical taps reach more than max_rows source rows (0: none)
int resample_tile_rows(const AxisTable *const *vertical, int nplanes, int max_rows) {
  for (int th = RESAMPLE_TH_MAX; th >= 1; th /= 2) {
    int widest = 0;
    for (int p = 0; p < nplanes; p++) vertical[p]->tile_spans(th, &widest);
    if (widest <= max_rows) return th;
  }
  return 0;
}

// device layout per axis: first [m], count [m], coef [maxcount][m], and for a vertical axis (the odd ones) its tiles' spans
int upload_axis_tables(const AxisTable *const *axes, int naxes, int th, int max_rows, DevBuf *dev, AxisTaps *out, hipStream_t stream) {
  std::vector<int32_t> host;
  size_t off[8][4];
  TM_CHECK(naxes >= 1 && naxes <= 8, TM_E_INVAL, "resample: %d axes", naxes);
  for (int a = 0; a < naxes; a++) {
    const AxisTable &t = *axes[a];
    int mc = 0;
    for (int j = 0; j < t.m; j++) mc = std::max(mc, t.count[j]);
    off[a][0] = host.size(); host.insert(host.end(), t.first.begin(), t.first.end());
    off[a][1] = host.size(); host.insert(host.end(), t.count.begin(), t.count.end());
    off[a][2] = host.size(); host.resize(host.size() + (size_t)mc * t.m);
    for (int k = 0; k < mc; k++)
      for (int j = 0; j < t.m; j++) host[off[a][2] + (size_t)k * t.m + j] = t.coef[(size_t)j * TM_RESAMPLE_MAX_TAPS + k];
    host.resize((host.size() + 1) & ~(size_t)1);  // (the spans are read as pairs)
    off[a][3] = host.size();
    if (a & 1) {
      int widest = 0;
      const std::vector<int32_t> sp = t.tile_spans(th, &widest);
      TM_CHECK(widest <= max_rows, TM_E_UNSUPPORTED, "resample: a tile reaches %d source rows", widest);  // (what resample_tile_rows chose th for)
      host.insert(host.end(), sp.begin(), sp.end());
    }
  }
  TM_HIP(hipStreamSynchronize(stream));  // a conversion in flight may still read the tables being replaced
  TM_TRY(dev->alloc(host.size() * 4));
  TM_HIP(hipMemcpyAsync(dev->p, host.data(), host.size() * 4, hipMemcpyHostToDevice, stream));
  TM_HIP(hipStreamSynchronize(stream));  // (`host` goes out of scope)
  for (int a = 0; a < naxes; a++)
    out[a] = AxisTaps{dev->as<int32_t>() + off[a][0], dev->as<int32_t>() + off[a][1], dev->as<int32_t>() + off[a][2], reinterpret_cast<const int2 *>(dev->as<int32_t>() + off[a][3])};
  return TM_OK;
}

}  // namespace tmx

extern "C" int tm_resample_taps_host(int n, int m, int np, int s, int o_halves, int32_t *first, int32_t *count, int32_t *coef) {
  TM_CHECK(first && count && coef, TM_E_INVAL, "null argument");
  return tmx::resample_taps(n, m, np, s, o_halves, first, count, coef, nullptr);
}
