// Bilinear resampling arithmetic shared by the stand-alone kernels (pointwise.hip) and the kernels that interpolate in flight (laf_fused.hip):
// one definition, so that a fused launch reproduces the stored map of the separate one bit for bit.
#pragma once

// F.interpolate(bilinear, align_corners=False): src = max(0, (dst+0.5)*in/out - 0.5), upper neighbour clamped
struct Lerp { int i0, i1; float l0, l1; };
// scale = (float)isz / (float)osz: one correctly rounded division, the same bits on the host and on the device
__device__ __forceinline__ Lerp lerp_of_r(int o, float scale, int isz) {
  float src = scale * ((float)o + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  int i0 = (int)src;
  if (i0 > isz - 1) i0 = isz - 1;
  int i1 = i0 + (i0 < isz - 1 ? 1 : 0);
  float l1 = src - (float)i0;
  return Lerp{i0, i1, 1.f - l1, l1};
}
__device__ __forceinline__ Lerp lerp_of(int o, int isz, int osz) { return lerp_of_r(o, (float)isz / (float)osz, isz); }

// one value from its four taps: columns first, then rows.
// bilerp_mix leaves the contraction into fma to the compiler (the Injection tail, whose surrounding arithmetic decides what is fused); bilerp_mix_fma
// writes the operations out - one product and one fma per row, one product and one fma across the rows - so that every kernel that uses it rounds
// at the same places: mgdt_bilinear_fwd and the kernels that must reproduce its stored map (laf_fused.hip).
__device__ __forceinline__ float bilerp_mix(float v00, float v01, float v10, float v11, Lerp ly, Lerp lx) {
  return (v00 * lx.l0 + v01 * lx.l1) * ly.l0 + (v10 * lx.l0 + v11 * lx.l1) * ly.l1;
}
__device__ __forceinline__ float bilerp_mix_fma(float v00, float v01, float v10, float v11, Lerp ly, Lerp lx) {
  const float r0 = fmaf(lx.l0, v00, lx.l1 * v01);
  const float r1 = fmaf(lx.l0, v10, lx.l1 * v11);
  return fmaf(r1, ly.l1, r0 * ly.l0);
}
