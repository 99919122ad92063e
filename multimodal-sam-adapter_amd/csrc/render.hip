// The picture of a prediction on device: what the reference's test loop does for `--show` / `--show-dir` (segmentation/mmseg_custom/apis/test_bs.py:257-349):
//   `tensor2imgs` (test_bs.py:18-63: mmcv.imdenormalize = cv2.multiply(std), cv2.add(mean), RGB->BGR when to_rgb; `* 255` when norm_by_max; .astype(uint8))
//   on planes 0..2 of the input tensor  ->  the crop to `img_shape` (test_bs.py:275-276)  ->  `show_result` (tools/color_gt_according_palette.py:23-81:
//   color_seg[seg == label] = color, the channels reversed, img * (1 - opacity) + color_seg * opacity in float64, .astype(uint8)).
// One pass, HBM-bound: uint8 class map [B, h, w] (any row / image stride) + a source -> uint8 HWC [B, h, w, 3].  The source is nothing (a black image),
// the raw uint8 HWC frame, or the normalised float32 NCHW tensor the backbone read.  The palette sits in LDS, one dword per entry (entries the palette
// does not have are 0: the reference's zero-initialised color_seg).  A lane owns 4 consecutive pixels of a row: pred as one dword, the raw frame as three
// dwords or the tensor as three float4, the 12 output bytes as three dwords; a workgroup covers 1024 pixels of one row.  Lanes whose 4 pixels are not
// aligned in pred (4 bytes), the raw frame (4), the tensor planes (16) or the output (4: its rows are 3 * w bytes, so the alignment changes from row to
// row unless w % 4 == 0), and the last lane of a width that is no multiple of 4, take the edge path, pixel by pixel.  Nothing outside any array is read.
#include "common.h"
#include "render_px.h"      // the blend, the de-normalisation and RenderDenorm: shared with csrc/render_diag.hip

// grid (cdiv(w, 1024), h, B).  src: RAW = uint8 [B, Hs, Ws, 3]; TENSOR = float32 [B, Cs, Hs, Ws]; both contiguous, the top-left h x w is used.
template <int SRC>
__global__ __launch_bounds__(256) void render_kernel(const unsigned char* __restrict__ pred, long pbs, long prs, const unsigned* __restrict__ palette,
                                                     int npal, int pal_rev, const void* __restrict__ src, int Cs, int Hs, int Ws, int src_rev,
                                                     RenderDenorm dn, double om, double op, unsigned char* __restrict__ out, int h, int w) {
  __shared__ unsigned pal[256];
  {
    unsigned v = (int)threadIdx.x < npal ? (palette[threadIdx.x] & 0xffffffu) : 0u;
    pal[threadIdx.x] = pal_rev ? render_swap02(v) : v;
  }
  __syncthreads();
  const int x = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
  if (x >= w) return;
  const int y = blockIdx.y, b = blockIdx.z;
  const int nvalid = min(4, w - x);
  const unsigned char* p = pred + (long)b * pbs + (long)y * prs + x;
  unsigned char* o = out + (((long)b * h + y) * w + x) * 3;
  const unsigned char* sr = nullptr;
  const float* st = nullptr;
  long plane = 0;
  bool vec = nvalid == 4 && ((((uintptr_t)p) | ((uintptr_t)o)) & 3u) == 0;
  if (SRC == RENDER_RAW) {
    sr = (const unsigned char*)src + (((long)b * Hs + y) * Ws + x) * 3;
    vec = vec && (((uintptr_t)sr) & 3u) == 0;
  }
  if (SRC == RENDER_TENSOR) {
    plane = (long)Hs * Ws;
    st = (const float*)src + (long)b * Cs * plane + (long)y * Ws + x;
    vec = vec && ((((uintptr_t)st) | ((uintptr_t)(plane * 4))) & 15u) == 0;
  }
  if (vec) {
    const unsigned pv = *(const unsigned*)p;
    unsigned s[4] = {0u, 0u, 0u, 0u};
    if (SRC == RENDER_RAW) {
      const unsigned* wv = (const unsigned*)sr;
      const unsigned w0 = wv[0], w1 = wv[1], w2 = wv[2];
      s[0] = w0 & 0xffffffu;
      s[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
      s[2] = (w1 >> 16) | ((w2 & 255u) << 16);
      s[3] = w2 >> 8;
      if (src_rev) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = render_swap02(s[q]);
      }
    }
    if (SRC == RENDER_TENSOR) {
      const float4 a = *(const float4*)st, g = *(const float4*)(st + plane), c = *(const float4*)(st + 2 * plane);
      s[0] = render_denorm(a.x, g.x, c.x, dn);
      s[1] = render_denorm(a.y, g.y, c.y, dn);
      s[2] = render_denorm(a.z, g.z, c.z, dn);
      s[3] = render_denorm(a.w, g.w, c.w, dn);
    }
    const unsigned q0 = render_pixel(s[0], pal[pv & 255u], om, op), q1 = render_pixel(s[1], pal[(pv >> 8) & 255u], om, op);
    const unsigned q2 = render_pixel(s[2], pal[(pv >> 16) & 255u], om, op), q3 = render_pixel(s[3], pal[pv >> 24], om, op);
    unsigned* ow = (unsigned*)o;
    ow[0] = q0 | (q1 << 24);
    ow[1] = (q1 >> 8) | (q2 << 16);
    ow[2] = (q2 >> 16) | (q3 << 8);
  } else {                                                                 // edge path: pixel by pixel
#pragma unroll 1
    for (int q = 0; q < nvalid; ++q) {
      unsigned s = 0u;
      if (SRC == RENDER_RAW) {
        s = (unsigned)sr[3 * q] | ((unsigned)sr[3 * q + 1] << 8) | ((unsigned)sr[3 * q + 2] << 16);
        if (src_rev) s = render_swap02(s);
      }
      if (SRC == RENDER_TENSOR) s = render_denorm(st[q], st[plane + q], st[2 * plane + q], dn);
      const unsigned v = render_pixel(s, pal[p[q]], om, op);
      o[3 * q] = (unsigned char)(v & 255u);
      o[3 * q + 1] = (unsigned char)((v >> 8) & 255u);
      o[3 * q + 2] = (unsigned char)(v >> 16);
    }
  }
}

static int render_check(const char* name, const unsigned char* pred, long pbs, long prs, int B, int h, int w, const unsigned* palette, int npal, double opacity,
                        double one_minus, const unsigned char* out) {
  MMSA_CHECK_ARG(pred && palette && out, "%s: null argument (pred, palette and out are required)", name);
  MMSA_CHECK_ARG(B > 0 && B <= 65535 && h > 0 && h <= 65535 && w > 0, "%s: bad map shape [%d, %d, %d]", name, B, h, w);
  MMSA_CHECK_ARG(prs >= w && (B == 1 || pbs >= (long)(h - 1) * prs + w), "%s: pred strides (image %ld, row %ld) overlap for a [%d, %d, %d] map", name, pbs, prs,
                 B, h, w);
  MMSA_CHECK_ARG(npal >= 1 && npal <= 256, "%s: a palette has 1..256 entries, got %d", name, npal);
  MMSA_CHECK_ARG(opacity > 0.0 && opacity <= 1.0 && one_minus >= 0.0 && one_minus < 1.0, "%s: opacity %g (1 - opacity %g) must be in (0, 1]", name, opacity,
                 one_minus);
  return MMSA_OK;
}

extern "C" int mmsa_render_u8(const unsigned char* pred, long pred_image_stride, long pred_row_stride, int B, int h, int w, const unsigned* palette, int npal,
                              int palette_reverse, const unsigned char* src, int Hs, int Ws, int src_reverse, double opacity, double one_minus_opacity,
                              unsigned char* out, hipStream_t stream) {
  int rc = render_check("render_u8", pred, pred_image_stride, pred_row_stride, B, h, w, palette, npal, opacity, one_minus_opacity, out);
  if (rc) return rc;
  const dim3 grid(cdiv(w, 1024), h, B), block(256);
  const RenderDenorm dn = {};
  if (src) {
    MMSA_CHECK_ARG(Hs >= h && Ws >= w, "render_u8: the %d x %d source is smaller than the %d x %d map", Hs, Ws, h, w);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(render_kernel<RENDER_RAW>), grid, block, 0, stream, pred, pred_image_stride, pred_row_stride, palette, npal,
                       palette_reverse != 0, (const void*)src, 3, Hs, Ws, src_reverse != 0, dn, one_minus_opacity, opacity, out, h, w);
  } else {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(render_kernel<RENDER_NONE>), grid, block, 0, stream, pred, pred_image_stride, pred_row_stride, palette, npal,
                       palette_reverse != 0, (const void*)nullptr, 0, 0, 0, 0, dn, one_minus_opacity, opacity, out, h, w);
  }
  MMSA_CHECK_LAUNCH("render_u8");
  return MMSA_OK;
}

extern "C" int mmsa_render_denorm_f32(const unsigned char* pred, long pred_image_stride, long pred_row_stride, int B, int h, int w, const unsigned* palette,
                                      int npal, int palette_reverse, const float* src, int Cs, int Hs, int Ws, const float* mean, const float* std, int to_rgb,
                                      int mul255, double opacity, double one_minus_opacity, unsigned char* out, hipStream_t stream) {
  int rc = render_check("render_denorm_f32", pred, pred_image_stride, pred_row_stride, B, h, w, palette, npal, opacity, one_minus_opacity, out);
  if (rc) return rc;
  MMSA_CHECK_ARG(src && mean && std, "render_denorm_f32: null argument (src, mean and std are required)");
  MMSA_CHECK_ARG(Cs >= 3, "render_denorm_f32: the tensor has %d planes, the picture needs the first 3", Cs);
  MMSA_CHECK_ARG(Hs >= h && Ws >= w, "render_denorm_f32: the %d x %d source is smaller than the %d x %d map", Hs, Ws, h, w);
  RenderDenorm dn;
  for (int c = 0; c < 3; ++c) { dn.mean[c] = mean[c]; dn.std[c] = std[c]; }
  dn.swap = to_rgb != 0;
  dn.mul255 = mul255 != 0;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(render_kernel<RENDER_TENSOR>), dim3(cdiv(w, 1024), h, B), dim3(256), 0, stream, pred, pred_image_stride, pred_row_stride,
                     palette, npal, palette_reverse != 0, (const void*)src, Cs, Hs, Ws, 0, dn, one_minus_opacity, opacity, out, h, w);
  MMSA_CHECK_LAUNCH("render_denorm_f32");
  return MMSA_OK;
}
