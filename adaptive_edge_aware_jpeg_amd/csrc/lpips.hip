// lpips.hip -- LPIPS(net='alex') of lpips 0.1.4 (evaluation_metrics.py:91-109) for a batch of image pairs: the AlexNet `features` trunk
// up to conv5's ReLU, taps after each of the five ReLUs, channel normalisation, the 1 x 1 "lin" weights and a spatial mean per tap.
//
// Convolutions: implicit GEMM on v_mfma_f32_32x32x2_f32.  M = output pixels, N = output channels, K = (ky, kx, cin); activations are NHWC
// float32.  A workgroup (4 waves) owns TH x 32 output pixels (TH = 4 * RW rows) x 64 channels: wave w computes rows w*RW .. w*RW+RW-1,
// each row one 32-pixel M tile, against two 32-channel N tiles (RW x 2 accumulators of 16 registers).  Per chunk of CK input channels
// the input window of the tile, halo included, is staged in LDS once (rows (TH-1)*S+KH, columns 31*S+KW, a pixel's CK channels at a
// stride of CK+1 words so the 32 lanes of a half-wave, one pixel each, fall into different banks); every (ky, kx) then reads its A
// fragments from that window.  The weights are packed by aej_lpips_pack_weights_host as [K][Cout] with K = (ky*KW + kx)*CinP + c, which is
// the B fragment order itself (lane l reads W[k0 + l/32][n0 + l%32]: 128 contiguous bytes per half-wave); they are read through L2.
// conv1's three input channels are padded to four (the fourth weight is zero) and the ScalingLayer is applied while staging its window.
// The epilogue adds the bias and applies the ReLU.
//
// Head: one wave per pixel, the lanes over the channels.  Both feature vectors are normalised (f / (sqrt(sum f^2) + 1e-10)) with a
// fixed butterfly reduction, d = sum_c w[c] (n0 - n1)^2 is reduced the same way, and each workgroup sums the d of a fixed range of pixels
// of one image in float64 in a fixed order into one partial.  k_lpips_final adds the partials of every tap in order: no atomics, so a
// result is the same from run to run and for an image alone or inside any batch.
#include "aej_common.h"
#include "aej_launch.h"
#include "aej_mfma.h"

#include <algorithm>

namespace aej {

// The five convolutions of AlexNet's `features` (torchvision): Cin, Cout, kernel, stride, padding; conv1's Cin padded to 4.
const LpipsLayer kLpipsLayers[kLpipsTaps] = {
    { 3, 4, 64, 11, 4, 2 }, { 64, 64, 192, 5, 1, 2 }, { 192, 192, 384, 3, 1, 1 }, { 384, 384, 256, 3, 1, 1 }, { 256, 256, 256, 3, 1, 1 },
};

bool lpips_geom(int H, int W, LpipsGeom &g)
{
    if (H < 31 || W < 31) return false;
    g.H = H; g.W = W;
    int h = (H + 2 * 2 - 11) / 4 + 1, w = (W + 2 * 2 - 11) / 4 + 1;          // conv1
    g.h[0] = h; g.w[0] = w;
    g.ph[0] = (h - 3) / 2 + 1; g.pw[0] = (w - 3) / 2 + 1;                      // maxpool 3/2 (floor)
    g.h[1] = g.ph[0]; g.w[1] = g.pw[0];                                        // conv2 (5 x 5, pad 2) keeps the size
    g.ph[1] = (g.h[1] - 3) / 2 + 1; g.pw[1] = (g.w[1] - 3) / 2 + 1;
    if (g.h[1] < 3 || g.w[1] < 3) return false;
    for (int l = 2; l < kLpipsTaps; l++) { g.h[l] = g.ph[1]; g.w[l] = g.pw[1]; }
    long long x = 0, y = 0, f = 0;
    for (int l = 0; l < kLpipsTaps; l++) {
        const long long n = (long long)g.h[l] * g.w[l] * kLpipsLayers[l].cout;
        g.tap_off[l] = f;
        f += (n + 63) / 64 * 64;
        g.nblk[l] = (int)(((long long)g.h[l] * g.w[l] + kLpipsHeadPixels - 1) / kLpipsHeadPixels);
        if (l == 3) y = n > y ? n : y; else x = n > x ? n : x;      // conv1, 2, 3, 5 write X, conv4 writes Y ...
    }
    for (int l = 0; l < 2; l++) y = std::max(y, (long long)g.ph[l] * g.pw[l] * kLpipsLayers[l].cout);     // ... and so do the pools
    g.x_elems = (x + 63) / 64 * 64;
    g.y_elems = (y + 63) / 64 * 64;
    g.feat_elems = f;
    g.max_blk = 0;
    for (int l = 0; l < kLpipsTaps; l++) g.max_blk = g.nblk[l] > g.max_blk ? g.nblk[l] : g.max_blk;
    return true;
}

long long lpips_packed_floats(long long off[kLpipsTaps][3])
{
    long long o = 0;
    for (int l = 0; l < kLpipsTaps; l++) {
        const LpipsLayer &L = kLpipsLayers[l];
        off[l][0] = o; o += (long long)L.k * L.k * L.cinp * L.cout;
        off[l][1] = o; o += L.cout;
        off[l][2] = o; o += L.cout;
        o = (o + 63) / 64 * 64;
    }
    return o;
}

long long lpips_param_floats()
{
    long long n = 0;
    for (int l = 0; l < kLpipsTaps; l++) {
        const LpipsLayer &L = kLpipsLayers[l];
        n += (long long)L.cout * L.cin * L.k * L.k + 2 * L.cout;
    }
    return n;
}

void lpips_pack_host(const float *params, float *packed)
{
    long long off[kLpipsTaps][3];
    const long long total = lpips_packed_floats(off);
    for (long long i = 0; i < total; i++) packed[i] = 0.f;
    const float *p = params;
    for (int l = 0; l < kLpipsTaps; l++) {                     // conv weights (OIHW) and biases
        const LpipsLayer &L = kLpipsLayers[l];
        float *w = packed + off[l][0];
        for (int o = 0; o < L.cout; o++)
            for (int c = 0; c < L.cin; c++)
                for (int ky = 0; ky < L.k; ky++)
                    for (int kx = 0; kx < L.k; kx++)
                        w[((long long)(ky * L.k + kx) * L.cinp + c) * L.cout + o] = p[((long long)(o * L.cin + c) * L.k + ky) * L.k + kx];
        p += (long long)L.cout * L.cin * L.k * L.k;
        for (int o = 0; o < L.cout; o++) packed[off[l][1] + o] = p[o];
        p += L.cout;
    }
    for (int l = 0; l < kLpipsTaps; l++) {                     // lin weights
        for (int o = 0; o < kLpipsLayers[l].cout; o++) packed[off[l][2] + o] = p[o];
        p += kLpipsLayers[l].cout;
    }
}

// ---- convolution ----------------------------------------------------------------------------------------------------------------
constexpr int kConvThreads = 256;

struct ConvArgs {
    const float *in;      // [B][IH][IW][Cin] (conv1: the images [B][H][W][3])
    const float *w;       // [KH*KW*CinP][Cout]
    const float *bias;    // [Cout]
    float *out;           // [B][OH][OW][Cout]
    int IH, IW, Cin, OH, OW, Cout, pad, tiles_x;
};

// lpips/pretrained_networks ScalingLayer after `x * 2 - 1`, in this operation order
__device__ __forceinline__ float lpips_scale_in(float x, int c)
{
    const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
    const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
    return (x * 2.0f - 1.0f - shift) / scale;
}

template <int KH, int KW, int S, int CK, int RW, bool RAW>
__global__ __launch_bounds__(kConvThreads) void k_lpips_conv(ConvArgs a)
{
    constexpr int TH = 4 * RW, WR = (TH - 1) * S + KH, WC = 31 * S + KW, CKP = CK + 1;
    constexpr int CINP = RAW ? 4 : 0;        // conv1 only: channels padded to 4 (a.Cin is the padded count for the others)
    __shared__ float win[WR * WC * CKP];
    const int tx0 = (blockIdx.x % a.tiles_x) * 32, ty0 = (blockIdx.x / a.tiles_x) * TH;
    const int n0 = blockIdx.y * 64, b = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, lh = lane >> 5;
    const int iy0 = ty0 * S - a.pad, ix0 = tx0 * S - a.pad;
    const int cinp = RAW ? CINP : a.Cin;
    const float *in = a.in + (long long)b * a.IH * a.IW * (RAW ? 3 : a.Cin);
    floatx16 acc[RW][2];
#pragma unroll
    for (int m = 0; m < RW; m++)
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;

    for (int c0 = 0; c0 < cinp; c0 += CK) {
        __syncthreads();
        for (int i = threadIdx.x; i < WR * WC * CK; i += kConvThreads) {
            const int c = i % CK, p = i / CK, col = p % WC, r = p / WC;
            const int iy = iy0 + r, ix = ix0 + col;
            float v = 0.f;
            if (iy >= 0 && iy < a.IH && ix >= 0 && ix < a.IW) {
                if (RAW) {
                    if (c < 3) v = lpips_scale_in(in[((long long)iy * a.IW + ix) * 3 + c], c);
                } else {
                    v = in[((long long)iy * a.IW + ix) * a.Cin + c0 + c];
                }
            }
            win[(r * WC + col) * CKP + c] = v;
        }
        __syncthreads();
        for (int ky = 0; ky < KH; ky++) {
            for (int kx = 0; kx < KW; kx++) {
                const float *wk = a.w + ((long long)(ky * KW + kx) * cinp + c0 + lh) * a.Cout + n0 + lr;
                float bf[CK / 2][2];
#pragma unroll
                for (int s = 0; s < CK / 2; s++)
#pragma unroll
                    for (int n = 0; n < 2; n++) bf[s][n] = wk[(long long)(2 * s) * a.Cout + n * 32];
                const float *wa = win + ((wave * RW * S + ky) * WC + lr * S + kx) * CKP + lh;
#pragma unroll
                for (int s = 0; s < CK / 2; s++) {
#pragma unroll
                    for (int m = 0; m < RW; m++) {
                        const float av = wa[m * S * WC * CKP + 2 * s];
#pragma unroll
                        for (int n = 0; n < 2; n++) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bf[s][n], acc[m][n], 0, 0, 0);
                    }
                }
            }
        }
    }
    // epilogue: bias + ReLU; lane lr holds channel n0 + n*32 + lr, register r pixel (r&3) + 8(r>>2) + 4 lh of the row
    float *out = a.out + (long long)b * a.OH * a.OW * a.Cout;
#pragma unroll
    for (int m = 0; m < RW; m++) {
        const int oy = ty0 + wave * RW + m;
        if (oy >= a.OH) continue;
#pragma unroll
        for (int n = 0; n < 2; n++) {
            const int ch = n0 + n * 32 + lr;
            const float bias = a.bias[ch];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int ox = tx0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (ox < a.OW) out[((long long)oy * a.OW + ox) * a.Cout + ch] = fmaxf(acc[m][n][r] + bias, 0.f);
            }
        }
    }
}

template <int KH, int KW, int S, int CK, int RW, bool RAW>
static void launch_conv(hipStream_t st, ConvArgs a, int B)
{
    constexpr int TH = 4 * RW;
    a.tiles_x = (a.OW + 31) / 32;
    const int tiles_y = (a.OH + TH - 1) / TH;
    hipLaunchKernelGGL((k_lpips_conv<KH, KW, S, CK, RW, RAW>), dim3(a.tiles_x * tiles_y, a.Cout / 64, B), dim3(kConvThreads), 0, st, a);
}

// ---- maxpool 3 / 2 (floor mode) -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lpips_pool(const float4 *__restrict__ in, float4 *__restrict__ out, int IH, int IW, int OH, int OW, int C4, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C4);
    long long p = i / C4;
    const int ox = (int)(p % OW);
    p /= OW;
    const int oy = (int)(p % OH);
    const long long b = p / OH;
    const float4 *src = in + ((b * IH + 2 * oy) * IW + 2 * ox) * C4 + c;
    float4 m = src[0];
    for (int dy = 0; dy < 3; dy++)
        for (int dx = 0; dx < 3; dx++) {
            const float4 v = src[((long long)dy * IW + dx) * C4];
            m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        }
    out[i] = m;
}

// ---- head -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// lpips.normalize_tensor: f / (sqrt(sum_c f^2) + 1e-10), NPL = C / 64 channels per lane (lane + 64 j)
template <int NPL>
__device__ __forceinline__ void lpips_normalise(float (&f)[NPL])
{
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NPL; j++) s += f[j] * f[j];
    const float nrm = sqrtf(wave_sum(s)) + 1e-10f;
#pragma unroll
    for (int j = 0; j < NPL; j++) f[j] = f[j] / nrm;
}

// grid (pixels / 4, B): one wave per pixel
template <int NPL>
__global__ __launch_bounds__(256) void k_lpips_normalise(const float *__restrict__ f, float *__restrict__ out, long long out_stride, long long npix)
{
    constexpr int C = 64 * NPL;
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npix) return;
    const float *F = f + blockIdx.y * npix * C;
    float *O = out + blockIdx.y * out_stride;
    float v[NPL];
#pragma unroll
    for (int j = 0; j < NPL; j++) v[j] = F[p * C + lane + 64 * j];
    lpips_normalise<NPL>(v);
#pragma unroll
    for (int j = 0; j < NPL; j++) O[p * C + lane + 64 * j] = v[j];
}

// grid (nblk, B): workgroup x of image b scores pixels [x * kLpipsHeadPixels, ...) of the tap; wave w takes pixels w, w + 4, ...
template <int NPL>
__global__ __launch_bounds__(256) void k_lpips_head(const float *__restrict__ na, long long a_stride, const float *__restrict__ fb, long long npix,
                                                    const float *__restrict__ lin, double *__restrict__ partial, int partial_stride)
{
    constexpr int C = 64 * NPL;
    __shared__ double wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const float *A = na + b * a_stride, *F = fb + b * npix * C;
    float w[NPL];
#pragma unroll
    for (int j = 0; j < NPL; j++) w[j] = lin[lane + 64 * j];
    double acc = 0.0;
    const long long p0 = (long long)blockIdx.x * kLpipsHeadPixels, p1 = p0 + kLpipsHeadPixels < npix ? p0 + kLpipsHeadPixels : npix;
    for (long long p = p0 + wave; p < p1; p += 4) {
        float x[NPL], y[NPL];
#pragma unroll
        for (int j = 0; j < NPL; j++) { x[j] = A[p * C + lane + 64 * j]; y[j] = F[p * C + lane + 64 * j]; }
        lpips_normalise<NPL>(y);
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < NPL; j++) { const float e = x[j] - y[j]; d += w[j] * (e * e); }
        acc += (double)wave_sum(d);
    }
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(long long)b * partial_stride + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// out[b] = sum over taps (in order) of (sum of the tap's partials, in order) / pixels of the tap
__global__ void k_lpips_final(const double *__restrict__ partial, int max_blk, LpipsGeom g, int B, double *__restrict__ out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double total = 0.0;
    for (int l = 0; l < kLpipsTaps; l++) {
        const double *p = partial + ((long long)b * kLpipsTaps + l) * max_blk;
        double s = 0.0;
        for (int i = 0; i < g.nblk[l]; i++) s += p[i];
        total += s / ((double)g.h[l] * g.w[l]);
    }
    out[b] = total;
}

template <int NPL>
static void launch_tap(hipStream_t st, int B, long long npix, const float *f, float *feats, long long feat_stride, const float *na, const float *lin,
                       double *partial, int nblk, int max_blk)
{
    if (feats) {     // features mode: the normalised tap of every image
        hipLaunchKernelGGL(k_lpips_normalise<NPL>, dim3((unsigned)((npix + 3) / 4), B), dim3(256), 0, st, f, feats, feat_stride, npix);
    } else {
        hipLaunchKernelGGL(k_lpips_head<NPL>, dim3(nblk, B), dim3(256), 0, st, na, feat_stride, f, npix, lin, partial, kLpipsTaps * max_blk);
    }
}

void launch_lpips(hipStream_t st, const float *wpk, const float *img, int B, const LpipsGeom &g, float *X, float *Y, float *feats_out,
                  const float *feats_a, double *partial, double *out)
{
    long long off[kLpipsTaps][3];
    lpips_packed_floats(off);
    const long long feat_stride = g.feat_elems;      // per image
    auto conv_args = [&](int l, const float *in, int IH, int IW, float *o) {
        ConvArgs a;
        a.in = in; a.w = wpk + off[l][0]; a.bias = wpk + off[l][1]; a.out = o;
        a.IH = IH; a.IW = IW; a.Cin = kLpipsLayers[l].cinp; a.OH = g.h[l]; a.OW = g.w[l]; a.Cout = kLpipsLayers[l].cout;
        a.pad = kLpipsLayers[l].pad; a.tiles_x = 0;
        return a;
    };
    auto tap = [&](int l, const float *f) {
        const long long npix = (long long)g.h[l] * g.w[l];
        float *fo = feats_out ? feats_out + g.tap_off[l] : nullptr;
        const float *na = feats_a ? feats_a + g.tap_off[l] : nullptr;
        const float *lin = wpk + off[l][2];
        double *part = partial ? partial + (long long)l * g.max_blk : nullptr;
        switch (kLpipsLayers[l].cout) {
        case 64: launch_tap<1>(st, B, npix, f, fo, feat_stride, na, lin, part, g.nblk[l], g.max_blk); break;
        case 192: launch_tap<3>(st, B, npix, f, fo, feat_stride, na, lin, part, g.nblk[l], g.max_blk); break;
        case 256: launch_tap<4>(st, B, npix, f, fo, feat_stride, na, lin, part, g.nblk[l], g.max_blk); break;
        default: launch_tap<6>(st, B, npix, f, fo, feat_stride, na, lin, part, g.nblk[l], g.max_blk); break;
        }
    };
    auto pool = [&](const float *in, int IH, int IW, int OH, int OW, int C, float *o) {
        const long long n = (long long)B * OH * OW * (C / 4);
        hipLaunchKernelGGL(k_lpips_pool, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float4 *>(in),
                           reinterpret_cast<float4 *>(o), IH, IW, OH, OW, C / 4, n);
    };
    // X / Y ping-pong: conv1 -> X, pool -> Y, conv2 -> X, pool -> Y, conv3 -> X, conv4 -> Y, conv5 -> X; each tap scored right away
    launch_conv<11, 11, 4, 4, 1, true>(st, conv_args(0, img, g.H, g.W, X), B);
    tap(0, X);
    pool(X, g.h[0], g.w[0], g.ph[0], g.pw[0], 64, Y);
    launch_conv<5, 5, 1, 32, 2, false>(st, conv_args(1, Y, g.ph[0], g.pw[0], X), B);
    tap(1, X);
    pool(X, g.h[1], g.w[1], g.ph[1], g.pw[1], 192, Y);
    launch_conv<3, 3, 1, 32, 2, false>(st, conv_args(2, Y, g.ph[1], g.pw[1], X), B);
    tap(2, X);
    launch_conv<3, 3, 1, 32, 2, false>(st, conv_args(3, X, g.h[2], g.w[2], Y), B);
    tap(3, Y);
    launch_conv<3, 3, 1, 32, 2, false>(st, conv_args(4, Y, g.h[3], g.w[3], X), B);
    tap(4, X);
    if (!feats_out) hipLaunchKernelGGL(k_lpips_final, dim3((B + 63) / 64), dim3(64), 0, st, partial, g.max_blk, g, B, out);
}

}  // namespace aej
