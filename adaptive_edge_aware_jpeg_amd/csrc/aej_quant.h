// aej_quant.h -- the quantiser of the codec, np.round(block / q).astype(int32) (jpeg.py:499-502), shared by the DCT epilogues
// (dct.hip) and the requantisation of stored DCT values (requant.hip).  One definition: both paths must give the same integer.
#pragma once
#include <hip/hip_runtime.h>

namespace aej {

// np.round(block / q).astype(int32): float64 quotient, round half to even (jpeg.py:499-502).
__device__ __forceinline__ int quantise_f64(float y, int q)
{
    double v = (double)y / (double)q;
    return (int)rint(v);
}

// The same integer from float32 operations only (the float64 division is ~15 double-rate instructions per coefficient and was
// the longest phase of the low-frequency wave of every large leaf).  k = rint(y * (1/q)) is at most one off; the remainder
// r = fma(-k, q, y) = y - k q is EXACT in float32 (it is a multiple of ulp(y) no larger than 1.5 q), so comparing |r| with q / 2
// decides between k and its neighbour, and |r| == q / 2 is exactly the case where the float64 quotient is k +- 1/2 and
// np.round goes to the even one.  (A non-zero |2r - q| is at least one ulp(y) >= 2^-24 |y|, far above the 2^-53 relative spacing
// at which the rounded float64 quotient could fake a tie.)  Range guard: quantisers above 2^22 or quotients above 2^18 -- never
// produced by the codec's own tables -- take the float64 division.  tests/native/quantise_check.c verifies the sequence, with the
// reciprocal perturbed by +-4 ulp, against rint((double)y / q) on 5e8 random, tie and near-tie cases.
__device__ __forceinline__ int quantise_f32(float y, float qf, float *quot = nullptr)      // qf = (float)q, q <= 2^22; valid while |y / q| < 2^18
{
    const float t = y * __builtin_amdgcn_rcpf(qf);
    const float k = __builtin_rintf(t);
    const float r = __builtin_fmaf(-k, qf, y);
    const float h = 0.5f * qf, ar = __builtin_fabsf(r);
    int ki = (int)k;
    if (ar > h || (ar == h && (ki & 1))) ki += r > 0.f ? 1 : -1;
    if (quot) *quot = t;
    return ki;
}

// quantise_f32 where it is proven, quantise_f64 for the whole wave as soon as one lane is outside its range
__device__ __forceinline__ int quantise(float y, int q)
{
    float t;
    const int ki = quantise_f32(y, (float)q, &t);
    const bool slow = q > (1 << 22) || !(__builtin_fabsf(t) < 262144.0f);
    if (__any(slow)) return quantise_f64(y, q);
    return ki;
}

}  // namespace aej
