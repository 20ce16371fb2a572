// jfif_arith.h -- the integer arithmetic of libjpeg's encoder that jfif.hip (one size per call) and jfifmany.hip (a size per image) share:
// RGB -> YCbCr (jccolor.c), h2v1 / h2v2 chroma down-sampling with the alternating bias (jcsample.c), the islow forward DCT (jfdctint.c)
// and the quantiser of its output (jcdctmgr.c).  Host + device, so that aej_jfif_many_coefs_host runs the code the kernels run.
// tests/jfif_reference.py is the same algorithm in numpy; tests/test_gpu_jfif*.py pin it to Pillow's files byte for byte.
#pragma once

#ifndef AEJ_HD
#define AEJ_HD __host__ __device__
#endif

namespace aej {

AEJ_HD __forceinline__ int jf_y(const unsigned char *p) { return (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16; }
AEJ_HD __forceinline__ int jf_c(const unsigned char *p, int comp)      // Cb (0) / Cr (1), libjpeg's rounding (ONE_HALF - 1)
{
    return comp == 0 ? (-11059 * p[0] - 21709 * p[1] + 32768 * p[2] + (128 << 16) + 32767) >> 16
                     : (32768 * p[0] - 27439 * p[1] - 5329 * p[2] + (128 << 16) + 32767) >> 16;
}
// chroma sample cx of a down-sampled row: the pixels at byte offsets x0, x1 (2 cx and 2 cx + 1, clamped to the last column by the
// caller) of one row (h2v1, bias 0, 1, 0, 1, ... from column 0) or of the row pair r0, r1 (h2v2, bias 1, 2, 1, 2, ...)
AEJ_HD __forceinline__ int jf_h2v1(const unsigned char *r0, int x0, int x1, int comp, int cx)
{
    return (jf_c(r0 + x0, comp) + jf_c(r0 + x1, comp) + (cx & 1)) >> 1;
}
AEJ_HD __forceinline__ int jf_h2v2(const unsigned char *r0, const unsigned char *r1, int x0, int x1, int comp, int cx)
{
    const int sum = jf_c(r0 + x0, comp) + jf_c(r0 + x1, comp) + jf_c(r1 + x0, comp) + jf_c(r1 + x1, comp);
    return (sum + 1 + (cx & 1)) >> 2;
}

AEJ_HD __forceinline__ long long jf_descale(long long x, int n) { return (x + (1LL << (n - 1))) >> n; }

// jfdctint, one 8-point pass over d[0], d[s], ..., d[7s]; pass 1 keeps PASS1_BITS of extra precision, pass 2 removes it
template <bool kPass1>
AEJ_HD __forceinline__ void jf_fdct8(long long *d, int s)
{
    const int n = kPass1 ? 11 : 15;
    long long t0 = d[0] + d[7 * s], t7 = d[0] - d[7 * s], t1 = d[s] + d[6 * s], t6 = d[s] - d[6 * s];
    long long t2 = d[2 * s] + d[5 * s], t5 = d[2 * s] - d[5 * s], t3 = d[3 * s] + d[4 * s], t4 = d[3 * s] - d[4 * s];
    long long t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = kPass1 ? (t10 + t11) * 4 : jf_descale(t10 + t11, 2);
    d[4 * s] = kPass1 ? (t10 - t11) * 4 : jf_descale(t10 - t11, 2);
    long long z1 = (t12 + t13) * 4433;
    d[2 * s] = jf_descale(z1 + t13 * 6270, n);
    d[6 * s] = jf_descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    long long z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7, z5 = (z3 + z4) * 9633;
    t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    d[7 * s] = jf_descale(t4 + z1 + z3, n);
    d[5 * s] = jf_descale(t5 + z2 + z4, n);
    d[3 * s] = jf_descale(t6 + z2 + z3, n);
    d[s] = jf_descale(t7 + z1 + z4, n);
}

AEJ_HD __forceinline__ int jf_quant(int c, int qt)      // libjpeg's quantiser of islow output: divisor 8 qt, rounded half away from zero
{
    const int q = qt << 3, a = ((c < 0 ? -c : c) + (q >> 1)) / q;
    return c < 0 ? -a : a;
}

}  // namespace aej
