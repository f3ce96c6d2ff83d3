// r3m_amd — on-GPU RandomResizedCrop resample for the `rc` / `rctraj` augmentations of the Ego4D loader
// (/root/reference/r3m/utils/data_loaders.py:47-50,81-102: transforms.RandomResizedCrop(224, scale=(0.2,1.0)) applied to
// x/255 and scaled back by 255; `rctraj` uses ONE box for the 5 stacked frames of a clip, `rc` one per frame).
// The crop boxes are inputs (drawn on the host with torchvision's get_params algorithm, r3m_amd/augment.py); this kernel
// is the crop + bilinear resize (align_corners=False, no antialias, as torchvision 0.8.2's tensor path) in one gather
// pass, uint8 or float frames in, float 0..255 out: HBM-bound, one read of the box region + one write.
#include "common.h"
#include "augment_dev.h"

namespace r3m {

template <typename T>
__global__ __launch_bounds__(256) void crop_resize_kernel(const T* __restrict__ in, const int* __restrict__ boxes,
                                                           float* __restrict__ out, long long total, int C, int Hi, int Wi,
                                                           int Ho, int Wo, int frames_per_box, int dst_top, int dst_left,
                                                           int full_Ho, int full_Wo) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int x = (int)(idx % Wo);
  long long t = idx / Wo;
  const int y = (int)(t % Ho); t /= Ho;
  const int c = (int)(t % C);
  const long long n = t / C;
  // box = source region (top, left, height, width); without boxes: the whole frame
  const int* b = boxes ? boxes + (n / frames_per_box) * 4 : nullptr;
  const int top = b ? b[0] : 0, left = b ? b[1] : 0, bh = b ? b[2] : Hi, bw = b ? b[3] : Wi;
  // The region is resized to full_Ho x full_Wo, of which this launch writes the Ho x Wo window at (dst_top, dst_left):
  // crop-then-resize has window == everything, resize-then-centre-crop has region == everything.
  const T* p = in + (n * C + c) * (long long)Hi * Wi;
  out[idx] = bilinear_sample(p, Wi, top, left, bh, bw, y, x, dst_top, dst_left, full_Ho, full_Wo);
}

static int launch_resample(const void* in, int in_is_u8, const int* boxes, float* out, long long N, int C, int Hi, int Wi, int Ho,
                           int Wo, int frames_per_box, int dst_top, int dst_left, int full_Ho, int full_Wo, hipStream_t s) {
  const long long total = N * C * Ho * Wo;
  if (total == 0) return 0;
  if (in_is_u8)
    hipLaunchKernelGGL((crop_resize_kernel<unsigned char>), dim3(ceil_div(total, 256)), dim3(256), 0, s,
                       static_cast<const unsigned char*>(in), boxes, out, total, C, Hi, Wi, Ho, Wo, frames_per_box, dst_top, dst_left,
                       full_Ho, full_Wo);
  else
    hipLaunchKernelGGL((crop_resize_kernel<float>), dim3(ceil_div(total, 256)), dim3(256), 0, s, static_cast<const float*>(in),
                       boxes, out, total, C, Hi, Wi, Ho, Wo, frames_per_box, dst_top, dst_left, full_Ho, full_Wo);
  return check_launch("crop_resize");
}

int launch_crop_resize(const void* in, int in_is_u8, const int* boxes, float* out, long long N, int C, int Hi, int Wi, int Ho,
                       int Wo, int frames_per_box, hipStream_t s) {
  R3M_REQUIRE(frames_per_box >= 1, "crop_resize: frames_per_box=%d", frames_per_box);
  // (two negative extents would make a positive element count, and a launch)
  R3M_REQUIRE(Hi >= 1 && Wi >= 1 && N >= 0 && C >= 1, "crop_resize: frames %lldx%dx%dx%d", N, C, Hi, Wi);
  R3M_REQUIRE(Ho >= 0 && Wo >= 0, "crop_resize: output %dx%d", Ho, Wo);
  return launch_resample(in, in_is_u8, boxes, out, N, C, Hi, Wi, Ho, Wo, frames_per_box, 0, 0, Ho, Wo, s);
}

// Resize(full) + crop of the Ho x Wo window at (top, left) in ONE pass: R3M.forward's Resize(256) + CenterCrop(224) branch for
// inputs that are not 224 x 224 (/root/reference/r3m/models/models_r3m.py:85-90). Only the window is ever computed.
int launch_resize_crop(const void* in, int in_is_u8, float* out, long long N, int C, int Hi, int Wi, int full_Ho, int full_Wo,
                       int top, int left, int Ho, int Wo, hipStream_t s) {
  R3M_REQUIRE(full_Ho >= 1 && full_Wo >= 1 && top >= 0 && left >= 0 && top + Ho <= full_Ho && left + Wo <= full_Wo,
              "resize_crop: window %dx%d at (%d,%d) outside the %dx%d resized frame", Ho, Wo, top, left, full_Ho, full_Wo);
  R3M_REQUIRE(Hi >= 1 && Wi >= 1 && N >= 0 && C >= 1, "resize_crop: frames %lldx%dx%dx%d", N, C, Hi, Wi);
  R3M_REQUIRE(Ho >= 0 && Wo >= 0, "resize_crop: window %dx%d", Ho, Wo);
  return launch_resample(in, in_is_u8, nullptr, out, N, C, Hi, Wi, Ho, Wo, 1, top, left, full_Ho, full_Wo, s);
}

// Adjoint of launch_resize_crop (float frames only): din[n,c,iy,ix] (= or +=) sum over the window pixels (y, x) whose bilinear taps
// include (iy, ix) of the tap weight times dout[n,c,y,x]. A GATHER — each input pixel visits the few window rows / columns whose
// source index lands next to it and re-derives their taps with bilinear_sample's own arithmetic — so there are no atomics and the
// result is the same bits on every run. The 1/255 and x255 of the forward cancel and are not applied.
struct ResizeAxis {
  int lo, hi;          // window indices [lo, hi) that may tap source index i
};
__device__ __forceinline__ ResizeAxis resize_axis_range(int i, float scale, int dst_off, int n_out) {
  // src = (dst + 0.5) scale - 0.5 in [i - 1, i + 1) <=> dst in [(i - 0.5) / scale - 0.5, (i + 1.5) / scale - 0.5): one index of
  // slack on each side, the exact test is made per candidate
  const int lo = (int)floorf(((float)i - 0.5f) / scale - 0.5f) - 1 - dst_off;
  const int hi = (int)ceilf(((float)i + 1.5f) / scale - 0.5f) + 2 - dst_off;
  return ResizeAxis{lo < 0 ? 0 : lo, hi > n_out ? n_out : hi};
}
// weight of source index i in the bilinear taps of window index d (bilinear_sample's arithmetic, contraction off)
__device__ __forceinline__ float resize_tap_weight(int d, int i, int dst_off, int in_len, int full_len) {
#pragma clang fp contract(off)
  const float sd = fmaxf(fmaf((float)(d + dst_off) + 0.5f, (float)in_len / (float)full_len, -0.5f), 0.f);
  const int i0 = (int)sd;
  const int i1 = i0 + (i0 < in_len - 1 ? 1 : 0);
  const float l = sd - (float)i0;
  float wgt = 0.f;
  if (i0 == i) wgt += 1.f - l;
  if (i1 == i) wgt += l;
  return wgt;
}

__global__ __launch_bounds__(256) void resize_crop_bwd_kernel(const float* __restrict__ dout, float* __restrict__ din, long long total,
                                                              int Hi, int Wi, int full_Ho, int full_Wo, int top, int left, int Ho,
                                                              int Wo, int accumulate) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;   // one thread per input pixel (n, c, iy, ix)
  if (idx >= total) return;
  const int ix = (int)(idx % Wi);
  const long long t = idx / Wi;
  const int iy = (int)(t % Hi);
  const long long nc = t / Hi;
  const ResizeAxis ry = resize_axis_range(iy, (float)Hi / (float)full_Ho, top, Ho);
  const ResizeAxis rx = resize_axis_range(ix, (float)Wi / (float)full_Wo, left, Wo);
  const float* g = dout + nc * Ho * Wo;
  float sum = 0.f;
  for (int y = ry.lo; y < ry.hi; ++y) {
    const float wy = resize_tap_weight(y, iy, top, Hi, full_Ho);
    if (wy == 0.f) continue;
    float row = 0.f;
    for (int x = rx.lo; x < rx.hi; ++x) {
      const float wx = resize_tap_weight(x, ix, left, Wi, full_Wo);
      if (wx != 0.f) row = fmaf(wx, g[(long long)y * Wo + x], row);
    }
    sum = fmaf(wy, row, sum);
  }
  din[idx] = accumulate ? din[idx] + sum : sum;
}

int launch_resize_crop_backward(const float* dout, float* din, long long N, int C, int Hi, int Wi, int full_Ho, int full_Wo, int top,
                                int left, int Ho, int Wo, int accumulate, hipStream_t s) {
  R3M_REQUIRE(full_Ho >= 1 && full_Wo >= 1 && top >= 0 && left >= 0 && top + Ho <= full_Ho && left + Wo <= full_Wo,
              "resize_crop_backward: window %dx%d at (%d,%d) outside the %dx%d resized frame", Ho, Wo, top, left, full_Ho, full_Wo);
  R3M_REQUIRE(Hi >= 1 && Wi >= 1 && N >= 0 && C >= 1, "resize_crop_backward: frames %lldx%dx%dx%d", N, C, Hi, Wi);
  const long long total = N * C * Hi * Wi;
  if (total == 0) return 0;
  hipLaunchKernelGGL(resize_crop_bwd_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, dout, din, total, Hi, Wi, full_Ho, full_Wo,
                     top, left, Ho, Wo, accumulate);
  return check_launch("resize_crop_backward");
}

}  // namespace r3m
