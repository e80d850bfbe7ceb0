// tm_render.hip -- the decoded frames on the device and their pixel-domain quality (PSNR, SSIM on luma) against the source.
//
// Render (tilingencoder.pas:3455-3640) with the constructor's defaults, the pictures GenerateY4M / GeneratePNGs export (tm_export.hip; handed to a caller by tm_render_api.hip):
// a predicted item copies 8 x 8 pixels of the previous output frame at its (clamped) offset, any other item is its palette-index tile
// (mirrored) looked up in its palette.  Pixels are 0x00RRGGBB, the format frames are pushed in.
//
// Predicted chains are resolved per pixel: a pixel of a predicted item moves to its source position in the frame before, until it lands on
// a drawn item (or before frame 0: black).  Every pixel is independent, so any frame range renders in one launch, whatever frames its
// chains reach back to (key frames end them: they hold no predicted items).  See DESIGN.md section 16.
#include "tm_common.h"
#include "tm_device.h"
#include "tm_internal.h"

namespace tmx {
namespace {

__device__ __forceinline__ uint32_t px_input(const RenderInput &in, int64_t f, int y, int x) {
  const int64_t i = f * ((int64_t)in.tm_w * in.tm_h) + (int64_t)(y >> 3) * in.tm_w + (x >> 3);
  const int fl = in.flags[i], ty = y & 7, tx = x & 7;
  return swap_rb(in.tiles[i * 64 + (((fl & 2) ? 7 - ty : ty) << 3) + ((fl & 1) ? 7 - tx : tx)]);
}

__device__ __forceinline__ uint32_t px_output(const RenderMap &m, int64_t f, int y, int x) {
  const int64_t per = (int64_t)m.tm_w * m.tm_h;
  const int sw = m.tm_w * 8, sh = m.tm_h * 8;
  for (; f >= 0; f--) {
    const int64_t i = f * per + (int64_t)(y >> 3) * m.tm_w + (x >> 3);
    if (m.pred && (m.pred[i] & m.pred_mask)) {  // Render 3595-3606: the back buffer (frame f - 1's output) at the predicted offset
      y = min(max(y + (int)m.py[i], 0), sh - 1);
      x = min(max(x + (int)m.px[i], 0), sw - 1);
      continue;
    }
    const int32_t t = m.tile[i], p = m.pal[i];
    if (t < 0 || t >= m.ntiles || p < 0 || p >= m.npal) return 0;
    const int fl = m.mir[i], ty = y & 7, tx = x & 7;
    const int c = m.pal_px[(int64_t)t * 64 + (((fl & 2) ? 7 - ty : ty) << 3) + ((fl & 1) ? 7 - tx : tx)];  // DrawTile, 3457-3503
    return c < m.pal_size ? swap_rb((uint32_t)m.palettes[(int64_t)p * m.pal_size + c]) : 0u;
  }
  return 0;  // before frame 0
}

__global__ __launch_bounds__(256) void k_render_output(RenderMap m, int first, int64_t n, uint32_t *__restrict__ out) {
  const int sw = m.tm_w * 8;
  const int64_t fpx = (int64_t)sw * m.tm_h * 8;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = e / fpx, r = e - f * fpx;
    const int y = (int)(r / sw), x = (int)(r - (int64_t)y * sw);
    out[e] = px_output(m, first + f, y, x);
  }
}

__global__ __launch_bounds__(256) void k_render_input(RenderInput in, int first, int64_t n, uint32_t *__restrict__ out) {
  const int sw = in.tm_w * 8;
  const int64_t fpx = (int64_t)sw * in.tm_h * 8;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = e / fpx, r = e - f * fpx;
    const int y = (int)(r / sw), x = (int)(r - (int64_t)y * sw);
    out[e] = px_input(in, first + f, y, x);
  }
}

// ---- quality: per 4 x 4 block the exact luma sums, per 8 x 8 window on the 4-pixel grid the SSIM term, per frame the RGB SSE
//
// One workgroup owns QB_R x QB_C blocks of one frame and computes one more row and column of blocks (its neighbours'), so that every
// window it owns -- blocks (r, c) .. (r + 1, c + 1) -- lies in its LDS.  Windows' SSIM terms are summed in a fixed order (workgroup
// tree, then frame_ssim_mean over the workgroups in order): the result does not depend on scheduling.  SSE goes through 64-bit integer atomics.
constexpr int QB_R = 4, QB_C = 50;  // (QB_R + 1) * (QB_C + 1) = 255 blocks: one per thread

// GenerateY4M's Y plane (tm_export.hip generate_y4m): RGBToYUV's y (utils.pas:478-490) in double narrowed to Single, rounded half to even
__device__ __forceinline__ int luma_y4m(uint32_t c /* 0x00RRGGBB */) {
  const int r = (c >> 16) & 0xff, g = (c >> 8) & 0xff, b = c & 0xff;
  const float yy = (float)(r * (299.0 / 1000) + g * (587.0 / 1000) + b * (114.0 / 1000));
  const double q = rint((double)yy);
  return q < 0 ? 0 : (q > 255 ? 255 : (int)q);
}

// The 16 pixels of the 4 x 4 block at block row br, block column bc of frame f, row-major, source in a[] and decoded in b[].
struct EncPair {  // source = the input render, decoded = the output render
  RenderInput in;
  RenderMap m;
  __device__ void block(int64_t f, int br, int bc, uint32_t a[16], uint32_t b[16]) const {
    // a block lies inside one item: its fields are read once, a source row is one 16-byte load
    const int64_t i = f * ((int64_t)in.tm_w * in.tm_h) + (int64_t)(br >> 1) * in.tm_w + (bc >> 1);
    const int y0 = (br & 1) * 4, x0 = (bc & 1) * 4;
    const int fi = in.flags[i];
    for (int r = 0; r < 4; r++) {
      const int ty = (fi & 2) ? 7 - (y0 + r) : y0 + r, tx = (fi & 1) ? 4 - x0 : x0;  // the row's four pixels, in stored order
      const uint4 v = *reinterpret_cast<const uint4 *>(in.tiles + i * 64 + ty * 8 + tx);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      for (int c = 0; c < 4; c++) a[r * 4 + c] = swap_rb(w[(fi & 1) ? 3 - c : c]);
    }
    if (m.pred && (m.pred[i] & m.pred_mask)) {  // predicted: every pixel traces its own chain
      for (int r = 0; r < 16; r++) b[r] = px_output(m, f, br * 4 + (r >> 2), bc * 4 + (r & 3));
      return;
    }
    const int32_t t = m.tile[i], p = m.pal[i];
    if (t < 0 || t >= m.ntiles || p < 0 || p >= m.npal) {
      for (int r = 0; r < 16; r++) b[r] = 0;
      return;
    }
    const int fl = m.mir[i];
    const int32_t *pal = m.palettes + (int64_t)p * m.pal_size;
    for (int r = 0; r < 4; r++) {
      const int ty = (fl & 2) ? 7 - (y0 + r) : y0 + r, tx = (fl & 1) ? 4 - x0 : x0;
      const uint32_t v = *reinterpret_cast<const uint32_t *>(m.pal_px + (int64_t)t * 64 + ty * 8 + tx);
      for (int c = 0; c < 4; c++) {
        const int k = (v >> (8 * ((fl & 1) ? 3 - c : c))) & 0xff;
        b[r * 4 + c] = k < m.pal_size ? swap_rb((uint32_t)pal[k]) : 0u;
      }
    }
  }
};
struct ImgPair {  // two stacks of frames [n][h][stride]
  const uint32_t *a, *b;
  int64_t stride, fstride;
  __device__ void block(int64_t f, int br, int bc, uint32_t pa[16], uint32_t pb[16]) const {
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) {
        const int64_t o = f * fstride + (int64_t)(br * 4 + r) * stride + bc * 4 + c;
        pa[r * 4 + c] = a[o];
        pb[r * 4 + c] = b[o];
      }
  }
};

template <class Pair>
__global__ __launch_bounds__(256) void k_frame_quality(Pair src, int first, int nbx, int nby, int ngx, int ngy,
                                                       unsigned long long *__restrict__ sse /* [n][3], zeroed */,
                                                       double *__restrict__ part /* [n][ngy][ngx] */) {
  __shared__ int4 s_blk[QB_R + 1][QB_C + 1];  // Sa, Sb, sum a^2 + b^2, sum ab
  __shared__ double s_red[256];
  __shared__ unsigned long long s_sse[4][3];
  const int tid = threadIdx.x;
  const int64_t wg = blockIdx.x;
  const int64_t f = wg / ((int64_t)ngx * ngy);
  const int g = (int)(wg - f * ngx * ngy), gy = g / ngx, gx = g - gy * ngx;
  const int br0 = gy * QB_R, bc0 = gx * QB_C;
  unsigned long long e0 = 0, e1 = 0, e2 = 0;
  if (tid < (QB_R + 1) * (QB_C + 1)) {
    const int sr = tid / (QB_C + 1), sc = tid - sr * (QB_C + 1), br = br0 + sr, bc = bc0 + sc;
    int4 s = make_int4(0, 0, 0, 0);
    if (br < nby && bc < nbx) {
      const bool own = sr < QB_R && sc < QB_C;
      uint32_t pa[16], pb[16];
      src.block(first + f, br, bc, pa, pb);
      for (int k = 0; k < 16; k++) {
          const uint32_t a = pa[k], b = pb[k];
          if (own) {
            const int d0 = (int)((a >> 16) & 0xff) - (int)((b >> 16) & 0xff), d1 = (int)((a >> 8) & 0xff) - (int)((b >> 8) & 0xff),
                      d2 = (int)(a & 0xff) - (int)(b & 0xff);
            e0 += (unsigned)(d0 * d0); e1 += (unsigned)(d1 * d1); e2 += (unsigned)(d2 * d2);
          }
          const int ya = luma_y4m(a), yb = luma_y4m(b);
          s.x += ya; s.y += yb; s.z += ya * ya + yb * yb; s.w += ya * yb;
        }
    }
    s_blk[sr][sc] = s;
  }
  // SSE: wave sums, then one atomic per channel per workgroup
  for (int o = 32; o > 0; o >>= 1) {
    e0 += __shfl_down(e0, o); e1 += __shfl_down(e1, o); e2 += __shfl_down(e2, o);
  }
  if ((tid & 63) == 0) { s_sse[tid >> 6][0] = e0; s_sse[tid >> 6][1] = e1; s_sse[tid >> 6][2] = e2; }
  __syncthreads();
  if (tid < 3) {
    const unsigned long long v = s_sse[0][tid] + s_sse[1][tid] + s_sse[2][tid] + s_sse[3][tid];
    if (v) atomicAdd(&sse[f * 3 + tid], v);
  }
  // windows (br0 + r, bc0 + c) this workgroup owns
  double w = 0.0;
  if (tid < QB_R * QB_C) {
    const int r = tid / QB_C, c = tid - r * QB_C;
    if (br0 + r < nby - 1 && bc0 + c < nbx - 1) {
      const int4 p = s_blk[r][c], q = s_blk[r][c + 1], u = s_blk[r + 1][c], v = s_blk[r + 1][c + 1];
      const int64_t sa = p.x + q.x + u.x + v.x, sb = p.y + q.y + u.y + v.y, sq = p.z + q.z + u.z + v.z, sp = p.w + q.w + u.w + v.w;
      const double c1 = 64.0 * 64.0 * (0.01 * 255) * (0.01 * 255), c2 = 64.0 * 64.0 * (0.03 * 255) * (0.03 * 255);
      const double num = (2.0 * (double)(sa * sb) + c1) * (2.0 * (double)(64 * sp - sa * sb) + c2);
      const double den = ((double)(sa * sa + sb * sb) + c1) * ((double)(64 * sq - sa * sa - sb * sb) + c2);
      w = num / den;
    }
  }
  s_red[tid] = w;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_red[tid] += s_red[tid + o];
    __syncthreads();
  }
  if (tid == 0) part[wg] = s_red[0];
}

// frame SSIM = the frame's window terms (its workgroups' partial sums, in order) over its window count
// (one wave per frame: lane l sums partials l, l + 64, ... in order, then a fixed butterfly)
__global__ __launch_bounds__(64) void k_frame_ssim_mean(const double *__restrict__ part, int per_frame, double nwin, double *__restrict__ ssim) {
  const int64_t f = blockIdx.x;
  double s = 0.0;
  for (int i = threadIdx.x; i < per_frame; i += 64) s += part[f * per_frame + i];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (threadIdx.x == 0) ssim[f] = s / nwin;
}

inline int grid_of(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256 * 64)); }

template <class Pair>
int run_quality(const Pair &src, int first, int n, int w, int h, void *sse, void *ssim, hipStream_t stream) {
  const int nbx = w / 4, nby = h / 4, ngx = (nbx + QB_C - 1) / QB_C, ngy = (nby + QB_R - 1) / QB_R;
  const int64_t nwg = (int64_t)n * ngx * ngy;
  TM_CHECK(nwg < (1ll << 31), TM_E_UNSUPPORTED, "frame quality: %lld workgroups", (long long)nwg);
  DevBuf part;  // (released at return: the pool hands memory back out in stream order, and everything here is on `stream`)
  TM_TRY(part.alloc((size_t)nwg * sizeof(double)));
  TM_HIP(hipMemsetAsync(sse, 0, (size_t)n * 3 * sizeof(uint64_t), stream));
  hipLaunchKernelGGL(k_frame_quality<Pair>, dim3((unsigned)nwg), dim3(256), 0, stream, src, first, nbx, nby, ngx, ngy, (unsigned long long *)sse,
                     part.as<double>());
  hipLaunchKernelGGL(k_frame_ssim_mean, dim3(n), dim3(64), 0, stream, part.as<double>(), ngx * ngy,
                     (double)(nbx - 1) * (double)(nby - 1), (double *)ssim);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

}  // namespace

int launch_render_output(const RenderMap &m, int first, int count, void *out, hipStream_t stream) {
  if (count <= 0) return TM_OK;
  const int64_t n = (int64_t)count * m.tm_w * 8 * m.tm_h * 8;
  hipLaunchKernelGGL(k_render_output, dim3(grid_of(n)), dim3(256), 0, stream, m, first, n, (uint32_t *)out);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

int launch_render_input(const RenderInput &in, int first, int count, void *out, hipStream_t stream) {
  if (count <= 0) return TM_OK;
  const int64_t n = (int64_t)count * in.tm_w * 8 * in.tm_h * 8;
  hipLaunchKernelGGL(k_render_input, dim3(grid_of(n)), dim3(256), 0, stream, in, first, n, (uint32_t *)out);
  TM_HIP(hipGetLastError());
  return TM_OK;
}

int launch_quality_render(const RenderInput &in, const RenderMap &m, int first, int count, void *sse, void *ssim, hipStream_t stream) {
  if (count <= 0) return TM_OK;
  EncPair p{in, m};
  return run_quality(p, first, count, m.tm_w * 8, m.tm_h * 8, sse, ssim, stream);
}

int launch_quality_frames(const void *a, const void *b, int n, int w, int h, int64_t stride_px, void *sse, void *ssim, hipStream_t stream) {
  TM_CHECK(a && b && sse && ssim && n >= 0 && w >= 8 && h >= 8 && w % 4 == 0 && h % 4 == 0 && stride_px >= w, TM_E_INVAL,
           "frame quality: bad arguments (frames of %d x %d, stride %lld: width and height must be multiples of 4, at least 8)", w, h, (long long)stride_px);
  if (n == 0) return TM_OK;
  ImgPair p{(const uint32_t *)a, (const uint32_t *)b, stride_px, stride_px * h};
  return run_quality(p, 0, n, w, h, sse, ssim, stream);
}

}  // namespace tmx
