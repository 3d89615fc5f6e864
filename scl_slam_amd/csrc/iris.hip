// iris.hip -- LiDAR-Iris building blocks on the GPU (include/scl_iris.h; reference include/descriptor.h:462-1302).
//
//   iris_image_kernel     getIris (D.h:532-598): one thread per point, atomicOr of the elevation bit into the
//                         (distance, yaw) cell, atomicMax of the height (order-preserving int image of the float;
//                         cells start at 0 like Eigen::MatrixXf::Zero, so only positive heights register);
//   iris_rowkey_kernel    row means in the reference's left-to-right float order;
//   (host, once)          the circular-convolution kernels of the four log-Gabor scales: response = idft(dft(x) * G)
//                         with both transforms unscaled (cv::dft / cv::idft without DFT_SCALE, D.h:651-653) equals
//                         x (*) h, h[n] = sum_k G[k] e^{2 pi i k n / N} -- computed in fp64 at engine creation;
//   iris_encode_kernel    logFeatureEncode (D.h:661-680): one workgroup per image column n, every (scale, row) response
//                         sum_m x[r][m] h_s[(n - m) mod N] in fp64 in index order, narrowed to float like the reference's
//                         planes, thresholded into the bit-packed templates: T / M as [column][20 words] bit masks over
//                         the 640 template rows, so a column shift is index arithmetic;
//   iris_hamming_kernel   getHammingDistance (D.h:932-964): one wave per (candidate, shift), popcounts of
//                         (T1s ^ T2) & ~(M1s | M2) and of the mask, integers end to end.
#include "scl_iris.h"

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "device_common.hpp"
#include "plugin_host.hpp"

using namespace scl;

namespace {

__device__ __forceinline__ int floor_to_int_x86(double v)
{
    const double f = floor(v);
    if (!(f >= -2147483648.0 && f <= 2147483647.0)) return (-2147483647 - 1);
    return (int)f;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void iris_image_kernel(const unsigned char *pts, int n, int stride, int rows, int cols, double add,
                                  unsigned int *cells /* rows*cols words: the byte image widened */, int *zmax)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float *f = reinterpret_cast<const float *>(pts + (size_t)i * (size_t)stride);
        const float x = f[0], y = f[1], z = f[2];
        const float dis = sqrtf(x * x + y * y);                                               // D.h:543
        const float arc = (float)((double)(iris_atan2f(z, dis) * 180.0f) / 3.14159265358979323846 + add);
        const float yaw = (float)((double)(iris_atan2f(y, x) * 180.0f) / 3.14159265358979323846 + 180);
        const int q_dis = clampi(floor_to_int_x86((double)dis), 0, rows - 1);
        const int q_arc = clampi(floor_to_int_x86((double)(arc / 4.0f)), 0, 7);
        const int q_yaw = clampi(floor_to_int_x86((double)yaw + 0.5), 0, cols - 1);
        const int cell = q_dis * cols + q_yaw;
        atomicOr(&cells[cell], 1u << q_arc);
        if (z > 0.0f) atomicMax(&zmax[cell], __float_as_int(z));      // positive floats order like their bit patterns; NaN never passes '<'
    }
}

__global__ void iris_rowkey_kernel(const int *zmax, const unsigned int *cells, int rows, int cols, float *rowkey, unsigned char *image)
{
    const int r = blockIdx.x;
    for (int c = threadIdx.x; c < cols; c += blockDim.x) image[(size_t)r * cols + c] = (unsigned char)cells[(size_t)r * cols + c];
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int c = 0; c < cols; ++c) s += __int_as_float(zmax[(size_t)r * cols + c]);
        rowkey[r] = s / (float)cols;
    }
}

// (kIrisWords = 20)                 // 640 template rows (2 * 4 scales * 80 rows) as 20 words per column

// one workgroup per image column n
__global__ __launch_bounds__(256) void iris_encode_kernel(const unsigned char *image, const double2 *h, int rows, int N, int nscale,
                                                          unsigned int *Tw, unsigned int *Mw /* [N][words] */, int words)
{
    extern __shared__ unsigned int lds_words[];             // [2 * words]
    const int n = blockIdx.x;
    for (int i = threadIdx.x; i < 2 * words; i += blockDim.x) lds_words[i] = 0u;
    __syncthreads();
    for (int job = threadIdx.x; job < nscale * rows; job += blockDim.x) {
        const int s = job / rows, r = job - s * rows;
        const unsigned char *xr = image + (size_t)r * N;
        const double2 *hs = h + (size_t)s * N;
        double re = 0.0, im = 0.0;
        for (int m = 0; m < N; ++m) {                       // index order, zeros skipped: the restatement's order
            const unsigned char xv = xr[m];
            if (xv == 0) continue;
            int d = n - m; d = d < 0 ? d + N : d;
            const double2 hv = hs[d];
            re += (double)xv * hv.x; im += (double)xv * hv.y;
        }
        const float fre = (float)re, fim = (float)im;
        const float mag = sqrtf(fre * fre + fim * fim);
        const int ta = s * rows + r, tb = (s + nscale) * rows + r;           // vconcat order, D.h:669-678
        if (fre > 0.0f) atomicOr(&lds_words[ta >> 5], 1u << (ta & 31));
        if (fim > 0.0f) atomicOr(&lds_words[tb >> 5], 1u << (tb & 31));
        if (mag < 0.0001f) { atomicOr(&lds_words[words + (ta >> 5)], 1u << (ta & 31)); atomicOr(&lds_words[words + (tb >> 5)], 1u << (tb & 31)); }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += blockDim.x) { Tw[(size_t)n * words + i] = lds_words[i]; Mw[(size_t)n * words + i] = lds_words[words + i]; }
}

__global__ void iris_unpack_kernel(const unsigned int *W, int N, int words, int trows, unsigned char *out /* [trows][N] */)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= trows * N) return;
    const int tr = i / N, n = i - tr * N;
    out[i] = (W[(size_t)n * words + (tr >> 5)] >> (tr & 31)) & 1u ? 255 : 0;
}

// one wave per (candidate, shift index); shift = shifts[job]
__global__ __launch_bounds__(64) void iris_hamming_kernel(const unsigned int *T, const unsigned int *M, size_t feat_words /* per keyframe */,
                                                          int key1, const int *cand, const int *shifts, int shifts_per_cand,
                                                          int N, int words, int trows, int *bits_diff, int *total_bits, const int *rolls2)
{
    const int job = blockIdx.x, c = job / shifts_per_cand;
    const int key2 = cand[c];
    int sh = shifts[job] % N; sh = sh < 0 ? sh + N : sh;
    int r2 = rolls2 ? rolls2[c] % N : 0; r2 = r2 < 0 ? r2 + N : r2;           // the second keyframe turned: circShift(T2, 0, roll), D.h:976-977
    const unsigned int *T1 = T + (size_t)key1 * feat_words, *M1 = M + (size_t)key1 * feat_words;
    const unsigned int *T2 = T + (size_t)key2 * feat_words, *M2 = M + (size_t)key2 * feat_words;
    int diff = 0, masked = 0;
    for (int i = threadIdx.x; i < N * words; i += 64) {
        const int k = i / words, w = i - k * words;
        int src = k - sh; src = src < 0 ? src + N : src;                       // circColShift: dst(:, k) = src(:, k - shift), D.h:581-592
        int k2 = k - r2; k2 = k2 < 0 ? k2 + N : k2;
        const unsigned int mask = M1[(size_t)src * words + w] | M2[(size_t)k2 * words + w];
        const unsigned int x = (T1[(size_t)src * words + w] ^ T2[(size_t)k2 * words + w]) & ~mask;
        diff += __popc(x); masked += __popc(mask);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { diff += __shfl_xor(diff, off, 64); masked += __shfl_xor(masked, off, 64); }
    if (threadIdx.x == 0) { bits_diff[job] = diff; total_bits[job] = trows * N - masked; }
}


// Row-key candidate search (libnabo's exact knn, D.h:1103-1109 / 1209-1215): squared L2 in fp32 between keyframe q's
// row key and those of list[0..n), accumulated four dimensions at a time and unfused -- the metric order the engine
// uses for every KD-tree search of the reference (ringkey_topk.hip; oracle nf_l2).  The k smallest are picked on the host.
__global__ void iris_rowkey_d2_kernel(const float *rowkeys, int rows, int q, const int *list, int n, float *d2)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *a = rowkeys + (size_t)q * rows, *b = rowkeys + (size_t)list[i] * rows;
    float result = 0.0f;
    int r = 0;
    for (; r + 3 < rows; r += 4) {
        const float d0 = __fsub_rn(a[r], b[r]), d1 = __fsub_rn(a[r + 1], b[r + 1]), d2v = __fsub_rn(a[r + 2], b[r + 2]), d3 = __fsub_rn(a[r + 3], b[r + 3]);
        const float t = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2v, d2v)), __fmul_rn(d3, d3));
        result = __fadd_rn(result, t);
    }
    for (; r < rows; ++r) { const float d0 = __fsub_rn(a[r], b[r]); result = __fadd_rn(result, __fmul_rn(d0, d0)); }
    d2[i] = result;
}


// ---- logPolarFFTTemplateMatch (D.h:793-925), the shift estimate in front of compare()'s Hamming windows -------------------------
// Restated from the algorithms OpenCV publishes (oracle/iris_oracle.c: iriso_fft_match states every step; PARITY UNPINNED against
// the reference's binaries).  Everything transcendental -- twiddles, the highpass, the log-polar map, the rotation matrix -- is
// evaluated on the host with the C library the CPU restatement uses and shipped as tables; the device adds, multiplies, divides and
// takes square roots, unfused, in the restatement's order: the two agree bit for bit.  J jobs (candidate, orientation) per launch.
struct FftJob { int key0, roll0, key1; };                  // im0 = image of key0 turned by roll0 columns, im1 = image of key1

// a[j][i] = (float)u8 * (float)(1 / 255)  (convertTo(CV_32FC1, 1.0 / 255.0), D.h:848-849)
__global__ void fm_stage_kernel(const unsigned char *images, const FftJob *jobs, int R, int C, float *a0, float *a1)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i >= R * C) return;
    const FftJob jb = jobs[j];
    const int r = i / C, c = i - r * C;
    int s0 = (c - jb.roll0) % C; s0 = s0 < 0 ? s0 + C : s0;                    // circShift(img, 0, roll): dst(:, c) = src(:, c - roll)
    const size_t n = (size_t)R * C;
    a0[(size_t)j * n + i] = (float)images[(size_t)jb.key0 * n + (size_t)r * C + s0] * (float)(1.0 / 255.0);
    a1[(size_t)j * n + i] = (float)images[(size_t)jb.key1 * n + i] * (float)(1.0 / 255.0);
}

__global__ void fm_to_complex_kernel(const float *src, double2 *dst, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[(size_t)blockIdx.y * n + i] = make_double2((double)src[(size_t)blockIdx.y * n + i], 0.0);
}

// out[l][k] = sum_m in[l][m] w^(k m): `lines` lines of n elements (element stride es, line stride ls); sgn -1 forward, +1 inverse.
// One thread per output; consecutive threads run along the dimension that is contiguous in memory.
__global__ __launch_bounds__(256) void fm_dft_lines_kernel(const double2 *in, double2 *out, int n, int es, int lines, int ls, int sgn,
                                                           const double *wc, const double *ws, size_t job_stride)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * lines) return;
    int k, l;
    if (es == 1) { l = t / n; k = t - l * n; } else { k = t / lines; l = t - k * lines; }
    const double2 *src = in + (size_t)blockIdx.y * job_stride + (size_t)l * ls;
    double re = 0.0, im = 0.0;
    int tw = 0;                                                                // (k * m) mod n
    for (int m = 0; m < n; ++m) {
        const double2 x = src[(size_t)m * es];
        const double c = wc[tw], s = sgn < 0 ? -ws[tw] : ws[tw];
        re = re + (x.x * c - x.y * s);
        im = im + (x.x * s + x.y * c);
        tw += k; tw = tw >= n ? tw - n : tw;
    }
    out[(size_t)blockIdx.y * job_stride + (size_t)l * ls + (size_t)k * es] = make_double2(re, im);
}

// recomb (quadrant swap), / (M N), magnitude on the float planes, highpass: f = |F| * h  (D.h:719-764, 856-872)
__global__ void fm_mag_highpass_kernel(const double2 *F, const float *hp, int R, int C, float *f)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * C) return;
    const int r = i / C, c = i - r * C;
    const size_t n = (size_t)R * C;
    const double2 v = F[(size_t)blockIdx.y * n + (size_t)((r + R / 2) % R) * C + (c + C / 2) % C];
    const float mn = (float)(R * C);
    const float re = (float)v.x / mn, im = (float)v.y / mn;
    f[(size_t)blockIdx.y * n + i] = sqrtf(re * re + im * im) * hp[i];
}

__device__ __forceinline__ float fm_bilinear32(const float *src, int R, int C, int sx, int sy)
{
    const int ix = sx >> 5, iy = sy >> 5, fx = sx & 31, fy = sy & 31;
    const float ax = (float)fx * (1.0f / 32.0f), ay = (float)fy * (1.0f / 32.0f);
    const float w00 = (1.0f - ax) * (1.0f - ay), w01 = ax * (1.0f - ay), w10 = (1.0f - ax) * ay, w11 = ax * ay;
    auto tap = [&](int yy, int xx) { return (yy >= 0 && yy < R && xx >= 0 && xx < C) ? src[(size_t)yy * C + xx] : 0.0f; };
    return ((tap(iy, ix) * w00 + tap(iy, ix + 1) * w01) + tap(iy + 1, ix) * w10) + tap(iy + 1, ix + 1) * w11;
}

// cv::remap through the log-polar map (fixed-point source positions from the host)
__global__ void fm_remap_kernel(const float *f, const int2 *map, int R, int C, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * C) return;
    const size_t n = (size_t)R * C;
    const int2 p = map[i];
    out[(size_t)blockIdx.y * n + i] = fm_bilinear32(f + (size_t)blockIdx.y * n, R, C, p.x, p.y);
}

// F1 conj(F2) / (|F1 conj(F2)| + FLT_EPSILON)
__global__ void fm_crosspower_kernel(const double2 *A, const double2 *B, double2 *out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double2 a = A[(size_t)blockIdx.y * n + i], b = B[(size_t)blockIdx.y * n + i];
    const double pr = a.x * b.x + a.y * b.y, pi = a.y * b.x - a.x * b.y;
    const double mag = sqrt(pr * pr + pi * pi) + (double)FLT_EPSILON;
    out[(size_t)blockIdx.y * n + i] = make_double2(pr / mag, pi / mag);
}

// quadrant swap, first maximum in row-major order, 5 x 5 weighted centroid: one workgroup per job; out = (cols / 2 - cx, rows / 2 - cy)
__global__ __launch_bounds__(256) void fm_peak_kernel(const double2 *Cr, int R, int C, double2 *out)
{
    const size_t n = (size_t)R * C;
    const double2 *src = Cr + (size_t)blockIdx.x * n;
    auto at = [&](int i, int j) { return (float)src[(size_t)((i + R / 2) % R) * C + (j + C / 2) % C].x; };
    float best = -INFINITY; int bidx = 0x7fffffff;
    for (int i = threadIdx.x; i < R * C; i += blockDim.x) {
        const float v = at(i / C, i % C);
        if (v > best) { best = v; bidx = i; }                                  // (ascending i per thread: the first maximum it meets)
    }
    __shared__ float sv[256]; __shared__ int si[256];
    sv[threadIdx.x] = best; si[threadIdx.x] = bidx;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const float ov = sv[threadIdx.x + off]; const int oi = si[threadIdx.x + off];
            if (ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < si[threadIdx.x])) { sv[threadIdx.x] = ov; si[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const int pr = si[0] == 0x7fffffff ? 0 : si[0] / C, pc = si[0] == 0x7fffffff ? 0 : si[0] % C;
    int minr = pr - 2, maxr = pr + 2, minc = pc - 2, maxc = pc + 2;
    minr = minr < 0 ? 0 : minr; minc = minc < 0 ? 0 : minc; maxr = maxr > R - 1 ? R - 1 : maxr; maxc = maxc > C - 1 ? C - 1 : maxc;
    double sum = 0.0, cx = 0.0, cy = 0.0;
    for (int y = minr; y <= maxr; ++y)
        for (int x = minc; x <= maxc; ++x) {
            const double v = (double)at(y, x);
            cx += (double)x * v; cy += (double)y * v; sum += v;
        }
    cx /= sum; cy /= sum;
    out[blockIdx.x] = make_double2((double)C / 2.0 - cx, (double)R / 2.0 - cy);
}

// cv::warpAffine with the inverted matrix in fixed point (AB_BITS 10, INTER_BITS 5): mats[j][6]
__global__ void fm_warp_kernel(const float *src, const double *mats, int R, int C, float *dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * C) return;
    const size_t n = (size_t)R * C;
    const double *M = mats + (size_t)blockIdx.y * 6;
    const int y = i / C, x = i - y * C;
    const int X0 = __double2int_rn((M[1] * (double)y + M[2]) * 1024.0) + 16, Y0 = __double2int_rn((M[4] * (double)y + M[5]) * 1024.0) + 16;
    const int X = (X0 + __double2int_rn(M[0] * (double)x * 1024.0)) >> 5, Y = (Y0 + __double2int_rn(M[3] * (double)x * 1024.0)) >> 5;
    dst[(size_t)blockIdx.y * n + i] = fm_bilinear32(src + (size_t)blockIdx.y * n, R, C, X, Y);
}


// ---- the batch forms (scl_iris.h "THE BATCH FORMS") ------------------------------------------------------------------------------
// The kernels below restate the single kernels over a launch group: integer results (cells, popcounts, bit words) are exact
// however they are partitioned, and every floating-point sum keeps the single kernel's order, so a batch call stores and answers
// the single calls' bits.  The single kernels above stay as they are: the tests hold these to them.
constexpr int kIrisMaxGroup = SCL_IRIS_MAX_GROUP, kIrisDetectGroup = SCL_IRIS_DETECT_GROUP;
constexpr int kEncodeStageBytes = 32 * 1024;               // image rows a workgroup of iris_encode_many_kernel holds in LDS at a time

// iris_image_kernel over a launch group: blockIdx.y = scan, its points at pts + offs[scan], its planes at scan * rows * cols
__global__ void iris_image_many_kernel(const unsigned char *pts, const unsigned long long *offs, const int *counts, int stride, int rows,
                                       int cols, double add, unsigned int *cells, int *zmax)
{
    const int g = blockIdx.y, n = counts[g];
    const unsigned char *p = pts + offs[g];
    unsigned int *cg = cells + (size_t)g * rows * cols;
    int *zg = zmax + (size_t)g * rows * cols;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float *f = reinterpret_cast<const float *>(p + (size_t)i * (size_t)stride);
        const float x = f[0], y = f[1], z = f[2];
        const float dis = sqrtf(x * x + y * y);
        const float arc = (float)((double)(iris_atan2f(z, dis) * 180.0f) / 3.14159265358979323846 + add);
        const float yaw = (float)((double)(iris_atan2f(y, x) * 180.0f) / 3.14159265358979323846 + 180);
        const int q_dis = clampi(floor_to_int_x86((double)dis), 0, rows - 1);
        const int q_arc = clampi(floor_to_int_x86((double)(arc / 4.0f)), 0, 7);
        const int q_yaw = clampi(floor_to_int_x86((double)yaw + 0.5), 0, cols - 1);
        const int cell = q_dis * cols + q_yaw;
        atomicOr(&cg[cell], 1u << q_arc);
        if (z > 0.0f) atomicMax(&zg[cell], __float_as_int(z));
    }
}

// grid (rows, scans): the byte image and the row key of scan g straight into database slot slot0 + g.  The heights of a row go
// through LDS so that the one thread that adds them, left to right as iris_rowkey_kernel does, reads them at LDS latency
__global__ __launch_bounds__(128) void iris_finish_many_kernel(const int *zmax, const unsigned int *cells, int rows, int cols, int slot0,
                                                               float *rowkeys, unsigned char *images)
{
    extern __shared__ float zrow[];                        // [cols]
    const int r = blockIdx.x, g = blockIdx.y;
    const size_t src = ((size_t)g * rows + r) * cols, slot = (size_t)slot0 + g;
    for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        images[(slot * rows + r) * cols + c] = (unsigned char)cells[src + c];
        zrow[c] = __int_as_float(zmax[src + c]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int c = 0; c < cols; ++c) s += zrow[c];
        rowkeys[slot * rows + r] = s / (float)cols;
    }
}

// iris_encode_kernel over a launch group: grid (cols, keyframes), the image of slot0 + blockIdx.y read from the database.  The image
// rows go through LDS, chunk_rows at a time (all of them where rows * cols fits kEncodeStageBytes: 28.8 KB at 80 x 360), as words of
// four pixels at a row pitch of whole words: a thread walks its row a word at a time and skips a zero word at once -- the pixels it
// does add come in ascending m with zeros skipped, iris_encode_kernel's sum.  LDS: [2 * words] bit words, then the rows
__global__ __launch_bounds__(256) void iris_encode_many_kernel(const unsigned char *images, const double2 *h, int rows, int N, int nscale,
                                                               unsigned int *T, unsigned int *M, int words, int slot0, int chunk_rows)
{
    extern __shared__ unsigned int lds_words[];
    const int n = blockIdx.x, pw = (N + 3) >> 2;
    const size_t slot = (size_t)slot0 + blockIdx.y;
    const unsigned char *image = images + slot * rows * N;
    unsigned int *img = lds_words + 2 * words;
    for (int i = threadIdx.x; i < 2 * words; i += blockDim.x) lds_words[i] = 0u;
    for (int r0 = 0; r0 < rows; r0 += chunk_rows) {
        const int rc = min(chunk_rows, rows - r0);
        __syncthreads();                                    // the bit words zeroed; the previous chunk read
        if ((N & 3) == 0) {                                 // rows start on words (slots and hipMalloc are aligned)
            const unsigned int *src = reinterpret_cast<const unsigned int *>(image + (size_t)r0 * N);
            for (int i = threadIdx.x; i < rc * pw; i += blockDim.x) img[i] = src[i];
        } else {
            unsigned char *ib = reinterpret_cast<unsigned char *>(img);
            for (int i = threadIdx.x; i < rc * pw * 4; i += blockDim.x) {
                const int rr = i / (pw * 4), c = i - rr * (pw * 4);
                ib[i] = c < N ? image[(size_t)(r0 + rr) * N + c] : (unsigned char)0;
            }
        }
        __syncthreads();
        for (int job = threadIdx.x; job < nscale * rc; job += blockDim.x) {
            const int s = job / rc, rr = job - s * rc, r = r0 + rr;
            const unsigned int *xw = img + rr * pw;
            const double2 *hs = h + (size_t)s * N;
            double re = 0.0, im = 0.0;
            for (int w = 0; w < pw; ++w) {
                const unsigned int v = xw[w];
                if (v == 0u) continue;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const unsigned int xv = (v >> (8 * b)) & 255u;
                    if (xv == 0u) continue;
                    int d = n - (4 * w + b); d = d < 0 ? d + N : d;
                    const double2 hv = hs[d];
                    re += (double)xv * hv.x; im += (double)xv * hv.y;
                }
            }
            const float fre = (float)re, fim = (float)im;
            const float mag = sqrtf(fre * fre + fim * fim);
            const int ta = s * rows + r, tb = (s + nscale) * rows + r;
            if (fre > 0.0f) atomicOr(&lds_words[ta >> 5], 1u << (ta & 31));
            if (fim > 0.0f) atomicOr(&lds_words[tb >> 5], 1u << (tb & 31));
            if (mag < 0.0001f) { atomicOr(&lds_words[words + (ta >> 5)], 1u << (ta & 31)); atomicOr(&lds_words[words + (tb >> 5)], 1u << (tb & 31)); }
        }
    }
    __syncthreads();
    const size_t out = (slot * N + n) * words;
    for (int i = threadIdx.x; i < words; i += blockDim.x) { T[out + i] = lds_words[i]; M[out + i] = lds_words[words + i]; }
}

// save_from_wire's decoder: grid (ceil((rows * cols + rows) / 256), vectors).  Pixel (r, c) from r * (cols + 1) + c + 1 (wire_decode 0,
// D.h:1035; the largest index read is rows * cols + rows - 1) or r * cols + c (1); float -> byte as x86 converts: out of int range
// or NaN -> 0, else truncation and the low byte.  The tests are explicit: the device's own conversion saturates.  The row key is copied
__global__ void iris_wire_decode_kernel(const float *values, int rows, int cols, int wire_decode, int slot0, unsigned char *images, float *rowkeys)
{
    const int cells = rows * cols, per = cells + rows;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per) return;
    const float *v = values + (size_t)blockIdx.y * per;
    const size_t slot = (size_t)slot0 + blockIdx.y;
    if (i < cells) {
        const int r = i / cols, c = i - r * cols;
        const float f = wire_decode ? v[(size_t)r * cols + c] : v[(size_t)r * (cols + 1) + c + 1];
        unsigned char b = 0;
        if (f > -2147483904.0f && f < 2147483648.0f) b = (unsigned char)((unsigned int)(int)f & 255u);
        images[slot * cells + i] = b;
    } else {
        rowkeys[slot * rows + (i - cells)] = v[i];
    }
}

// iris_rowkey_d2_kernel for up to kIrisDetectGroup queries that share one candidate list (nn_l2_many_kernel's scheme): query q is
// keyframe qkey[q] against the prefix list[0 .. limit[q]); a thread owns one candidate, reads its row key once and keeps the
// queries' running sums in registers, each in iris_rowkey_d2_kernel's order.  LDS: the queries' row keys, [kIrisDetectGroup][rows]
__global__ __launch_bounds__(256) void iris_rowkey_d2_many_kernel(const float *rowkeys, int rows, const int *qkey, const int *limit, int nq,
                                                                  const int *list, int n, float *d2 /* [nq][d2_stride] */, int d2_stride)
{
    extern __shared__ float qs[];
    for (int e = threadIdx.x; e < kIrisDetectGroup * rows; e += blockDim.x) {
        const int q = e / rows;
        qs[e] = q < nq ? rowkeys[(size_t)qkey[q] * rows + (e - q * rows)] : 0.0f;
    }
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *b = rowkeys + (size_t)list[i] * rows;
    float result[kIrisDetectGroup];
#pragma unroll
    for (int q = 0; q < kIrisDetectGroup; ++q) result[q] = 0.0f;
    int r = 0;
    for (; r + 3 < rows; r += 4) {
        const float b0 = b[r], b1 = b[r + 1], b2 = b[r + 2], b3 = b[r + 3];
#pragma unroll
        for (int q = 0; q < kIrisDetectGroup; ++q) {
            const float *a = qs + q * rows + r;
            const float d0 = __fsub_rn(a[0], b0), d1 = __fsub_rn(a[1], b1), d2v = __fsub_rn(a[2], b2), d3 = __fsub_rn(a[3], b3);
            const float t = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2v, d2v)), __fmul_rn(d3, d3));
            result[q] = __fadd_rn(result[q], t);
        }
    }
    for (; r < rows; ++r) {
        const float b0 = b[r];
#pragma unroll
        for (int q = 0; q < kIrisDetectGroup; ++q) {
            const float d0 = __fsub_rn(qs[q * rows + r], b0);
            result[q] = __fadd_rn(result[q], __fmul_rn(d0, d0));
        }
    }
#pragma unroll
    for (int q = 0; q < kIrisDetectGroup; ++q)
        if (q < nq && i < limit[q]) d2[(size_t)q * d2_stride + i] = result[q];
}

// The candidate selection of detect_core_locked, one workgroup per query: the m smallest squared distances of d2[q][0 .. limit[q])
// in ascending order, equal ones by ascending position; d <= eps is skipped when eps > 0 and !(d < FLT_MAX) never enters.  What
// enters is a non-negative finite float, whose bits order as integers: round c takes the smallest 64-bit (distance bits, position)
// key above round c - 1's.  cand_pos[q][c] = the position, -1 from the first round that finds nothing
__global__ __launch_bounds__(256) void iris_select_kernel(const float *d2, int d2_stride, const int *limit, int m, float eps, int *cand_pos)
{
    __shared__ unsigned long long part[4];
    const int q = blockIdx.x, n = limit[q];
    const float *d = d2 + (size_t)q * d2_stride;
    unsigned long long prev = 0ull;
    for (int c = 0; c < m; ++c) {
        unsigned long long best = ~0ull;
        for (int i = threadIdx.x; i < n; i += 256) {
            const float v = d[i];
            if (eps > 0.0f && v <= eps) continue;
            if (!(v < FLT_MAX)) continue;
            const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned int)i;
            if ((c == 0 || key > prev) && key < best) best = key;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off, 64);
            best = o < best ? o : best;
        }
        __syncthreads();                                    // the previous round's partials read
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
        __syncthreads();
        best = part[0];
        for (int w = 1; w < 4; ++w) best = part[w] < best ? part[w] : best;
        if (best == ~0ull) {                                // uniform over the workgroup
            for (int j = c + threadIdx.x; j < m; j += 256) cand_pos[(size_t)q * m + j] = -1;
            return;
        }
        if (threadIdx.x == 0) cand_pos[(size_t)q * m + c] = (int)(best & 0xffffffffu);
        prev = best;
    }
}

// cand_pos -> the candidates' global keys and, with passes > 0, compare()'s FftJob list on the device: per (query, candidate) the
// pass against the candidate as it is and / or turned by 180 columns (roll_first: the roll of the first pass run).  An empty
// candidate slot gives key -1 and jobs with key0 = -1, which every later kernel skips.  One thread per (query, candidate)
__global__ void iris_jobs_kernel(const int *cand_pos, const int *qkey, const int *list_off, const int *list, int nq, int m, int passes,
                                 int roll_first, int *cand_key, FftJob *jobs)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * m) return;
    const int q = i / m, pos = cand_pos[i];
    const int key = pos < 0 ? -1 : list[list_off[q] + pos];
    cand_key[i] = key;
    for (int p = 0; p < passes; ++p) jobs[(size_t)i * passes + p] = FftJob{key, p == 0 ? roll_first : 180, qkey[q]};
}

// fm_stage_kernel with the job list made on the device: an empty job (key0 < 0) stages zeros, so that the transforms behind it read
// nothing undefined; its estimate is never used
__global__ void fm_stage_many_kernel(const unsigned char *images, const FftJob *jobs, int R, int C, float *a0, float *a1)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i >= R * C) return;
    const FftJob jb = jobs[j];
    const size_t n = (size_t)R * C;
    if (jb.key0 < 0) { a0[(size_t)j * n + i] = 0.0f; a1[(size_t)j * n + i] = 0.0f; return; }
    const int r = i / C, c = i - r * C;
    int s0 = (c - jb.roll0) % C; s0 = s0 < 0 ? s0 + C : s0;
    a0[(size_t)j * n + i] = (float)images[(size_t)jb.key0 * n + (size_t)r * C + s0] * (float)(1.0 / 255.0);
    a1[(size_t)j * n + i] = (float)images[(size_t)jb.key1 * n + i] * (float)(1.0 / 255.0);
}

// compare()'s Hamming window of one job per workgroup: the query jobs[j].key1 shifted by est[j] - 2 .. est[j] + 2 against the
// candidate jobs[j].key0 turned by roll0 columns, as iris_hamming_kernel takes them.  The candidate's T / M words are read once, the
// query's once per shift (five neighbouring columns); (diff, total) per shift to [j][5]
__global__ __launch_bounds__(256) void iris_hamming_window_kernel(const unsigned int *T, const unsigned int *M, size_t feat_words, const FftJob *jobs,
                                                                  const int *est, int N, int words, int trows, int *bits_diff, int *total_bits)
{
    __shared__ int part[4][10];
    const int j = blockIdx.x;
    const FftJob jb = jobs[j];
    if (jb.key0 < 0) return;
    int sh[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) { int s = (int)((unsigned int)est[j] - 2u + (unsigned int)t) % N; sh[t] = s < 0 ? s + N : s; }
    int r2 = jb.roll0 % N; r2 = r2 < 0 ? r2 + N : r2;
    const unsigned int *T1 = T + (size_t)jb.key1 * feat_words, *M1 = M + (size_t)jb.key1 * feat_words;
    const unsigned int *T2 = T + (size_t)jb.key0 * feat_words, *M2 = M + (size_t)jb.key0 * feat_words;
    int acc[10];
#pragma unroll
    for (int t = 0; t < 10; ++t) acc[t] = 0;
    for (int i = threadIdx.x; i < N * words; i += 256) {
        const int k = i / words, w = i - k * words;
        int k2 = k - r2; k2 = k2 < 0 ? k2 + N : k2;
        const unsigned int t2 = T2[(size_t)k2 * words + w], m2 = M2[(size_t)k2 * words + w];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            int src = k - sh[t]; src = src < 0 ? src + N : src;
            const unsigned int mask = M1[(size_t)src * words + w] | m2;
            acc[t] += __popc((T1[(size_t)src * words + w] ^ t2) & ~mask); acc[5 + t] += __popc(mask);
        }
    }
#pragma unroll
    for (int t = 0; t < 10; ++t) {
        for (int off = 32; off > 0; off >>= 1) acc[t] += __shfl_xor(acc[t], off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][t] = acc[t];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int t = threadIdx.x;
        bits_diff[(size_t)j * 5 + t] = part[0][t] + part[1][t] + part[2][t] + part[3][t];
        total_bits[(size_t)j * 5 + t] = trows * N - (part[0][5 + t] + part[1][5 + t] + part[2][5 + t] + part[3][5 + t]);
    }
}

// shift_search = 1: iris_hamming_kernel with the query per candidate slot -- one wave per (slot, column shift), slot = query * m + c
__global__ __launch_bounds__(64) void iris_hamming_all_many_kernel(const unsigned int *T, const unsigned int *M, size_t feat_words, const int *qkey,
                                                                   const int *cand_key, int m, int N, int words, int trows, int *bits_diff, int *total_bits)
{
    const int job = blockIdx.x, slot = job / N, sh = job - slot * N;
    const int key2 = cand_key[slot];
    if (key2 < 0) return;
    const int key1 = qkey[slot / m];
    const unsigned int *T1 = T + (size_t)key1 * feat_words, *M1 = M + (size_t)key1 * feat_words;
    const unsigned int *T2 = T + (size_t)key2 * feat_words, *M2 = M + (size_t)key2 * feat_words;
    int diff = 0, masked = 0;
    for (int i = threadIdx.x; i < N * words; i += 64) {
        const int k = i / words, w = i - k * words;
        int src = k - sh; src = src < 0 ? src + N : src;
        const unsigned int mask = M1[(size_t)src * words + w] | M2[i];
        diff += __popc((T1[(size_t)src * words + w] ^ T2[i]) & ~mask); masked += __popc(mask);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { diff += __shfl_xor(diff, off, 64); masked += __shfl_xor(masked, off, 64); }
    if (threadIdx.x == 0) { bits_diff[job] = diff; total_bits[job] = trows * N - masked; }
}

// what a batched detection answers per query: the best candidate's position in the query's list (-1: none), its shift and distance
struct IrisAnswer { int pos, bias; float dis; };

// One thread per query of the launch group, the host's steps behind the Hamming counts: per job the selection over its shifts
// (hamming_jobs_locked: cur = diff / total correctly rounded; total == 0 resets the running best to NaN in window mode and is
// skipped in the exhaustive mode; else cur < best || isnan(best)), compare()'s merge by match_num in C's integer arithmetic, and
// the best candidate in candidate order with strict < from 10000000 (a NaN never wins).  window: per = 5 shifts est - 2 + t and
// `passes` jobs per candidate; else per = N shifts t and one job per candidate
__global__ void iris_finish_detect_kernel(const int *cand_pos, const int *est, const int *bits_diff, const int *total_bits, int nq, int m, int per,
                                          int window, int passes, int match_num, IrisAnswer *out)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    IrisAnswer a = {-1, 0, 10000000.0f};
    for (int c = 0; c < m; ++c) {
        const size_t slot = (size_t)q * m + c;
        if (cand_pos[slot] < 0) break;                      // the empty slots trail
        float ds[2] = {0.0f, 0.0f}; int bs[2] = {0, 0};
        for (int p = 0; p < passes; ++p) {
            const size_t j = slot * passes + p;
            float best = NAN; int b = -1;
            for (int t = 0; t < per; ++t) {
                const int total = total_bits[j * per + t];
                if (total == 0) { if (window) best = NAN; continue; }
                const float cur = __fdiv_rn((float)bits_diff[j * per + t], (float)total);
                if (cur < best || isnan(best)) { best = cur; b = window ? (int)((unsigned int)est[j] - 2u + (unsigned int)t) : t; }
            }
            ds[p] = best; bs[p] = b;
        }
        float dis = ds[0]; int bias = bs[0];
        if (window && match_num == 2) { if (!(ds[0] < ds[1])) { dis = ds[1]; bias = (bs[1] + 180) % 360; } }     // D.h:986-997
        else if (window && match_num == 1) bias = (bs[0] + 180) % 360;                                            // the one pass run is the second
        if (dis < a.dis) { a.dis = dis; a.pos = cand_pos[slot]; a.bias = bias; }
    }
    out[q] = a;
}

// ---- the exhaustive ranked search (scl_iris.h "THE EXHAUSTIVE SEARCH") ----------------------------------------------------------
// iris_search_score_kernel: one workgroup per candidate of the search set, one LANE per column shift.  iris_hamming_kernel pairs
// the query's column k - s with the candidate's column k; over k' = k - s that is the query's column k' with the candidate's column
// (k' + s) mod N.  So at every step all lanes need the SAME query word -- a uniform address, which the compiler serves with scalar
// loads from L2: the queries of a launch group are 16 x 57.6 KB at the defaults -- and lane s needs the candidate word s columns
// further on, which comes from LDS, where the workgroup stages its candidate once: {T, M} pairs as [column][pitch], pitch = words | 1
// pairs, so that the 32 lanes of a ds_read_b64 group, one column apart, fall on 32 different bank pairs.  Every pair a lane reads from
// LDS serves kSearchQuad queries; a candidate crosses HBM once per launch group whatever the number of shifts and queries.  A lane
// keeps its shift's two integer counts per query in registers over all N * words words, so nothing is reduced per shift; per pair
// the (score bits << 32 | shift) keys of the shifts with total != 0 are reduced to their minimum -- the first minimum, scores being
// non-negative floats -- and only (score, shift) leaves the kernel: NaN and -1 where every shift is fully masked.
// kLds = false: a template that does not fit kSearchLdsBytes is read from global memory instead, column by column per lane.
constexpr int kSearchQuad = 4;                             // queries a lane scores per candidate word it reads
constexpr int kSearchMaxThreads = 512;                     // lanes = shifts rounded up to whole waves, at most this (more shifts: passes)
constexpr size_t kSearchLdsBytes = 64 * 1024 - 256;        // the staged candidate (60 480 B at 80 x 360: two workgroups per CU); 256 B: `part`

template <bool kLds>
__global__ __launch_bounds__(kSearchMaxThreads) void iris_search_score_kernel(const unsigned int *__restrict__ T, const unsigned int *__restrict__ M,
                                                                               size_t feat_words, const int *__restrict__ qkey,
                                                                               const int *__restrict__ limit, int nq, const int *__restrict__ list,
                                                                               int N, int words, int trows, float *__restrict__ score,
                                                                               int *__restrict__ bias, int stride)
{
    extern __shared__ uint2 cand_lds[];                    // [N][pitch] {T, M} (kLds)
    __shared__ unsigned long long part[kSearchQuad][kSearchMaxThreads / 64];
    const int pos = blockIdx.x, tid = threadIdx.x, pitch = words | 1;
    const size_t c_off = (size_t)list[pos] * feat_words;
    const unsigned int *T2 = T + c_off, *M2 = M + c_off;
    if (kLds) {
        for (int i = tid; i < N * words; i += blockDim.x) {
            const int k = i / words, w = i - k * words;
            cand_lds[k * pitch + w] = make_uint2(T2[i], M2[i]);
        }
        __syncthreads();
    }
    for (int q0 = 0; q0 < nq; q0 += kSearchQuad) {
        bool act[kSearchQuad], any = false;
        const unsigned int *Tq[kSearchQuad], *Mq[kSearchQuad];
#pragma unroll
        for (int j = 0; j < kSearchQuad; ++j) {
            act[j] = q0 + j < nq && pos < limit[q0 + j];
            any = any || act[j];
            const size_t q_off = act[j] ? (size_t)qkey[q0 + j] * feat_words : c_off;       // an idle slot scores the candidate itself, unused
            Tq[j] = T + q_off; Mq[j] = M + q_off;
        }
        if (!any) continue;                                 // the same for every lane
        unsigned long long best[kSearchQuad];
#pragma unroll
        for (int j = 0; j < kSearchQuad; ++j) best[j] = ~0ull;
        for (int s0 = 0; s0 < N; s0 += blockDim.x) {
            const bool live = s0 + tid < N;
            const int s = live ? s0 + tid : 0;
            int diff[kSearchQuad], masked[kSearchQuad];
#pragma unroll
            for (int j = 0; j < kSearchQuad; ++j) { diff[j] = 0; masked[j] = 0; }
            int col = s;                                    // the candidate's column under the query's column k
            for (int k = 0; k < N; ++k) {
                const size_t qo = (size_t)k * words;
                const uint2 *cl = cand_lds + col * pitch;
                const unsigned int *ct = T2 + (size_t)col * words, *cm = M2 + (size_t)col * words;
#pragma unroll 4
                for (int w = 0; w < words; ++w) {
                    const uint2 c = kLds ? cl[w] : make_uint2(ct[w], cm[w]);
#pragma unroll
                    for (int j = 0; j < kSearchQuad; ++j) {
                        const unsigned int mask = Mq[j][qo + w] | c.y;
                        diff[j] += __popc((Tq[j][qo + w] ^ c.x) & ~mask); masked[j] += __popc(mask);
                    }
                }
                col = col + 1 == N ? 0 : col + 1;
            }
#pragma unroll
            for (int j = 0; j < kSearchQuad; ++j) {
                const int total = trows * N - masked[j];
                if (live && total != 0) {
                    const unsigned long long key = ((unsigned long long)__float_as_uint(__fdiv_rn((float)diff[j], (float)total)) << 32) | (unsigned int)s;
                    best[j] = key < best[j] ? key : best[j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kSearchQuad; ++j) {
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(best[j], off, 64);
                best[j] = o < best[j] ? o : best[j];
            }
            if ((tid & 63) == 0) part[j][tid >> 6] = best[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kSearchQuad; ++j) {
            if (tid != j || !act[j]) continue;
            unsigned long long b = part[j][0];
            for (int w = 1; w < (int)(blockDim.x >> 6); ++w) b = part[j][w] < b ? part[j][w] : b;
            const size_t o = (size_t)(q0 + j) * stride + pos;
            score[o] = b == ~0ull ? NAN : __uint_as_float((unsigned int)(b >> 32));
            bias[o] = b == ~0ull ? -1 : (int)(b & 0xffffffffu);
        }
        __syncthreads();                                    // part read before the next quad writes it
    }
}

// one ranked entry of a query: its position in the query's search set (-1: the slot is unused), the shift and the score
struct IrisSearchEntry { int pos, bias; float dis; };

// cand_pos (iris_select_kernel over the scores) -> the entries of a launch group: one thread per (query, rank)
__global__ void iris_search_finish_kernel(const int *cand_pos, const float *score, const int *bias, int stride, int nq, int k, IrisSearchEntry *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * k) return;
    const int q = i / k, pos = cand_pos[i];
    IrisSearchEntry e = {-1, 0, INFINITY};
    if (pos >= 0) { e.pos = pos; e.bias = bias[(size_t)q * stride + pos]; e.dis = score[(size_t)q * stride + pos]; }
    out[i] = e;
}

}  // namespace

namespace {

// a device work buffer of the batch forms: regrown on demand (nothing is kept), never shrunk
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;                                            // bytes
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// The batch forms' own work buffers: the single calls never see them, and a later single call finds its buffers as it left them
struct IrisBatchWork {
    DevBuf points, planes, table;                              // builders: a group's clouds, its cell | zmax planes, the offset | count tables
    DevBuf wire;                                               // save_from_wire_many: the vectors as received
    DevBuf list, query, d2, cand, jobs, est, counts, answers;  // detections
    DevBuf fm, fres, fmats;                                    // FFT shift estimate: the work planes of one pass, its results and matrices
    DevBuf sscore, sbias, spos, sres;                          // exhaustive search: a group's scores and shifts, the ranked positions, the entries
    void release()
    {
        for (DevBuf *b : {&points, &planes, &table, &wire, &list, &query, &d2, &cand, &jobs, &est, &counts, &answers, &fm, &fres, &fmats, &sscore, &sbias,
                          &spos, &sres}) {
            if (b->p) (void)hipFree(b->p);
            b->p = nullptr; b->cap = 0;
        }
    }
};

}  // namespace

struct scl_iris {
    IrisBatchWork bw;
    scl_iris_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    mutable std::mutex mu;
    mutable std::string last_error;
    scl::KeyframeRegistry reg;
    int cap = 0;                                               // rows of the image / row key / template store (reg.n live)
    int words = 0, trows = 0;
    unsigned char *d_images = nullptr; float *d_rowkeys = nullptr; unsigned int *d_T = nullptr, *d_M = nullptr;
    double2 *d_h = nullptr;
    unsigned int *d_cells = nullptr; int *d_zmax = nullptr; unsigned char *d_points = nullptr; size_t points_cap = 0;
    unsigned char *d_img1 = nullptr; float *d_key1 = nullptr; unsigned char *d_unpack = nullptr;
    int *d_cand = nullptr, *d_shifts = nullptr, *d_diff = nullptr, *d_total = nullptr; size_t job_cap = 0;
    int *d_list = nullptr; float *d_d2 = nullptr; size_t list_cap = 0;
    // FFT shift estimate (logPolarFFTTemplateMatch): tables made at creation, work buffers for fm_cap jobs
    double *d_wcR = nullptr, *d_wsR = nullptr, *d_wcC = nullptr, *d_wsC = nullptr; float *d_hp = nullptr; int2 *d_lpmap = nullptr; float log_base = 0.f;
    bool fm_ok = false;                                        // even rows / cols (the restatement's quadrant swap)
    size_t fm_cap = 0;
    FftJob *d_fjobs = nullptr; float *d_fa0 = nullptr, *d_fa1 = nullptr, *d_ff = nullptr, *d_flp0 = nullptr, *d_flp1 = nullptr, *d_frs = nullptr;
    double2 *d_fw0 = nullptr, *d_fw1 = nullptr, *d_fw2 = nullptr, *d_fres = nullptr; double *d_fmats = nullptr;
    int *d_rolls = nullptr; size_t rolls_cap = 0;
};

namespace {

int grow(scl_iris *h, int need)
{
    if (need <= h->cap) return SCL_OK;
    int ncap = h->cap > 0 ? h->cap : 256;
    while (ncap < need) ncap *= 2;
    const size_t cells = (size_t)h->cfg.rows * h->cfg.cols, fw = (size_t)h->cfg.cols * h->words;
    unsigned char *ni = nullptr; float *nk = nullptr; unsigned int *nt = nullptr, *nm = nullptr;
    int rc;
    if ((rc = dev_alloc(h, &ni, cells * ncap)) || (rc = dev_alloc(h, &nk, (size_t)h->cfg.rows * ncap)) || (rc = dev_alloc(h, &nt, fw * ncap)) || (rc = dev_alloc(h, &nm, fw * ncap))) return rc;
    if (h->reg.n > 0) {
        SCL_HIP(h, hipMemcpyAsync(ni, h->d_images, cells * h->reg.n, hipMemcpyDeviceToDevice, h->stream));
        SCL_HIP(h, hipMemcpyAsync(nk, h->d_rowkeys, sizeof(float) * h->cfg.rows * h->reg.n, hipMemcpyDeviceToDevice, h->stream));
        SCL_HIP(h, hipMemcpyAsync(nt, h->d_T, sizeof(unsigned int) * fw * h->reg.n, hipMemcpyDeviceToDevice, h->stream));
        SCL_HIP(h, hipMemcpyAsync(nm, h->d_M, sizeof(unsigned int) * fw * h->reg.n, hipMemcpyDeviceToDevice, h->stream));
    }
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    if (h->d_images) (void)hipFree(h->d_images);
    if (h->d_rowkeys) (void)hipFree(h->d_rowkeys);
    if (h->d_T) (void)hipFree(h->d_T);
    if (h->d_M) (void)hipFree(h->d_M);
    h->d_images = ni; h->d_rowkeys = nk; h->d_T = nt; h->d_M = nm; h->cap = ncap;
    return SCL_OK;
}

// points (host) -> d_img1 / d_key1
int make_image_locked(scl_iris *h, const void *points, int n_points, int stride)
{
    if (n_points < 0 || stride < 12 || (stride & 3) || (n_points > 0 && !points)) return fail(h, SCL_ERR_INVALID_ARG, "bad point layout");
    const int rows = h->cfg.rows, cols = h->cfg.cols;
    const size_t bytes = (size_t)n_points * stride;
    if (bytes > h->points_cap) {
        h->points_cap = 0;
        int rc = dev_regrow(h, &h->d_points, bytes + bytes / 4 + 4096);
        if (rc) return rc;
        h->points_cap = bytes + bytes / 4 + 4096;
    }
    if (bytes) SCL_HIP(h, hipMemcpyAsync(h->d_points, points, bytes, hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemsetAsync(h->d_cells, 0, sizeof(unsigned int) * (size_t)rows * cols, h->stream));
    SCL_HIP(h, hipMemsetAsync(h->d_zmax, 0, sizeof(int) * (size_t)rows * cols, h->stream));
    if (n_points > 0 && (h->cfg.nscan == 16 || h->cfg.nscan == 64)) {             // D.h:538 / 560: other beam counts leave the image empty
        int blocks = (n_points + 255) / 256; blocks = blocks > 2048 ? 2048 : blocks;
        hipLaunchKernelGGL(iris_image_kernel, dim3(blocks), dim3(256), 0, h->stream, h->d_points, n_points, stride, rows, cols,
                           h->cfg.nscan == 16 ? 15.0 : 24.9, h->d_cells, h->d_zmax);
    }
    hipLaunchKernelGGL(iris_rowkey_kernel, dim3(rows), dim3(128), 0, h->stream, h->d_zmax, h->d_cells, rows, cols, h->d_key1, h->d_img1);
    SCL_HIP(h, hipGetLastError());
    return SCL_OK;
}

// d_img1 / d_key1 -> database slot n (image, row key, templates)
int append_locked(scl_iris *h, int8_t robot, int index)
{
    int rc;
    if ((rc = check_robot(h, robot, SCL_ERR_INVALID_ARG)) || (rc = grow(h, h->reg.n + 1))) return rc;
    const int rows = h->cfg.rows, cols = h->cfg.cols;
    const size_t cells = (size_t)rows * cols, fw = (size_t)cols * h->words;
    SCL_HIP(h, hipMemcpyAsync(h->d_images + cells * h->reg.n, h->d_img1, cells, hipMemcpyDeviceToDevice, h->stream));
    SCL_HIP(h, hipMemcpyAsync(h->d_rowkeys + (size_t)rows * h->reg.n, h->d_key1, sizeof(float) * rows, hipMemcpyDeviceToDevice, h->stream));
    hipLaunchKernelGGL(iris_encode_kernel, dim3(cols), dim3(256), sizeof(unsigned int) * 2 * h->words, h->stream,
                       h->d_img1, h->d_h, rows, cols, h->cfg.nscale, h->d_T + fw * h->reg.n, h->d_M + fw * h->reg.n, h->words);
    SCL_HIP(h, hipGetLastError());
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    h->reg.commit(robot, index);                                                  // D.h:1055-1057
    return SCL_OK;
}

int hamming_jobs_locked(scl_iris *h, int key1, const int *cand, const int *shifts, int n, int per, float *dis, int *bias, bool window, const int *rolls2 = nullptr)
{
    if (key1 < 0 || key1 >= h->reg.n) return fail(h, SCL_ERR_OUT_OF_RANGE, "key1 out of range");
    for (int i = 0; i < n; ++i) if (cand[i] < 0 || cand[i] >= h->reg.n) return fail(h, SCL_ERR_OUT_OF_RANGE, "candidate out of range");
    const size_t jobs = (size_t)n * per;
    if (jobs > h->job_cap) {
        for (int **p : {&h->d_cand, &h->d_shifts, &h->d_diff, &h->d_total}) { if (*p) (void)hipFree(*p); *p = nullptr; }
        h->job_cap = 0;
        int rc;
        if ((rc = dev_alloc(h, &h->d_cand, jobs + 64)) || (rc = dev_alloc(h, &h->d_shifts, jobs + 64)) || (rc = dev_alloc(h, &h->d_diff, jobs + 64)) || (rc = dev_alloc(h, &h->d_total, jobs + 64))) return rc;
        h->job_cap = jobs + 64;
    }
    SCL_HIP(h, hipMemcpyAsync(h->d_cand, cand, sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemcpyAsync(h->d_shifts, shifts, sizeof(int) * jobs, hipMemcpyHostToDevice, h->stream));
    if (rolls2) {
        if ((size_t)n > h->rolls_cap) {
            h->rolls_cap = 0;
            int rc = dev_regrow(h, &h->d_rolls, (size_t)n + 64);
            if (rc) return rc;
            h->rolls_cap = (size_t)n + 64;
        }
        SCL_HIP(h, hipMemcpyAsync(h->d_rolls, rolls2, sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
    }
    const size_t fw = (size_t)h->cfg.cols * h->words;
    hipLaunchKernelGGL(iris_hamming_kernel, dim3((unsigned)jobs), dim3(64), 0, h->stream, h->d_T, h->d_M, fw, key1, h->d_cand, h->d_shifts, per,
                       h->cfg.cols, h->words, h->trows, h->d_diff, h->d_total, rolls2 ? h->d_rolls : (const int *)nullptr);
    SCL_HIP(h, hipGetLastError());
    std::vector<int> diff(jobs), total(jobs);
    SCL_HIP(h, hipMemcpyAsync(diff.data(), h->d_diff, sizeof(int) * jobs, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipMemcpyAsync(total.data(), h->d_total, sizeof(int) * jobs, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    for (int c = 0; c < n; ++c) {                                             // the O(shifts) selection of D.h:937-962, float like the reference
        float best = NAN; int b = -1;
        for (int j = 0; j < per; ++j) {
            const size_t job = (size_t)c * per + j;
            if (total[job] == 0) { if (window) best = NAN; continue; }        // D.h:948-951 resets dis; the exhaustive form just skips
            const float cur = (float)diff[job] / (float)total[job];
            if (cur < best || std::isnan(best)) { best = cur; b = shifts[job]; }
        }
        dis[c] = best; bias[c] = b;
    }
    return SCL_OK;
}

// fftMatch for J jobs: centre x of the RotatedRect as a float (D.h:927-932); ok[j] = 0 where the reference prints "Images are not
// compatible" and returns an empty rectangle (centre 0).  Two round trips to the host: the rotation / scale of the log-polar stage
// and the translation.
int fft_match_jobs_locked(scl_iris *h, const FftJob *jobs, int J, float *center_x, int *ok_out)
{
    if (J <= 0) return SCL_OK;
    if (!h->fm_ok) return fail(h, SCL_ERR_UNSUPPORTED, "the FFT shift estimate takes even rows and columns only");
    const int R = h->cfg.rows, C = h->cfg.cols;
    const size_t n = (size_t)R * C;
    if ((size_t)J > h->fm_cap) {
        for (void **p : {(void **)&h->d_fjobs, (void **)&h->d_fa0, (void **)&h->d_fa1, (void **)&h->d_ff, (void **)&h->d_flp0, (void **)&h->d_flp1, (void **)&h->d_frs,
                         (void **)&h->d_fw0, (void **)&h->d_fw1, (void **)&h->d_fw2, (void **)&h->d_fres, (void **)&h->d_fmats}) { if (*p) (void)hipFree(*p); *p = nullptr; }
        h->fm_cap = 0;
        const size_t cap = (size_t)J + 8;
        int rc;
        if ((rc = dev_alloc(h, &h->d_fjobs, cap)) || (rc = dev_alloc(h, &h->d_fa0, cap * n)) || (rc = dev_alloc(h, &h->d_fa1, cap * n)) || (rc = dev_alloc(h, &h->d_ff, cap * n)) ||
            (rc = dev_alloc(h, &h->d_flp0, cap * n)) || (rc = dev_alloc(h, &h->d_flp1, cap * n)) || (rc = dev_alloc(h, &h->d_frs, cap * n)) || (rc = dev_alloc(h, &h->d_fw0, cap * n)) ||
            (rc = dev_alloc(h, &h->d_fw1, cap * n)) || (rc = dev_alloc(h, &h->d_fw2, cap * n)) || (rc = dev_alloc(h, &h->d_fres, cap)) || (rc = dev_alloc(h, &h->d_fmats, cap * 6))) return rc;
        h->fm_cap = cap;
    }
    hipStream_t st = h->stream;
    const dim3 ge((unsigned)((n + 255) / 256), (unsigned)J), blk(256);
    SCL_HIP(h, hipMemcpyAsync(h->d_fjobs, jobs, sizeof(FftJob) * (size_t)J, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(fm_stage_kernel, ge, blk, 0, st, h->d_images, h->d_fjobs, R, C, h->d_fa0, h->d_fa1);
    // 2-D DFT of a float image: rows, then columns; result in w_out, w_tmp as scratch
    auto dft2 = [&](const float *src, double2 *w_out, double2 *w_tmp) {
        hipLaunchKernelGGL(fm_to_complex_kernel, ge, blk, 0, st, src, w_tmp, (int)n);
        hipLaunchKernelGGL(fm_dft_lines_kernel, ge, blk, 0, st, w_tmp, w_out, C, 1, R, C, -1, h->d_wcC, h->d_wsC, n);
        hipLaunchKernelGGL(fm_dft_lines_kernel, ge, blk, 0, st, w_out, w_tmp, R, C, C, 1, -1, h->d_wcR, h->d_wsR, n);
        (void)hipMemcpyAsync(w_out, w_tmp, sizeof(double2) * n * (size_t)J, hipMemcpyDeviceToDevice, st);
    };
    auto phase_correlate = [&](const float *s1, const float *s2) {             // -> d_fres[j] = (tx, ty)
        dft2(s1, h->d_fw0, h->d_fw2);
        dft2(s2, h->d_fw1, h->d_fw2);
        hipLaunchKernelGGL(fm_crosspower_kernel, ge, blk, 0, st, h->d_fw0, h->d_fw1, h->d_fw2, (int)n);
        hipLaunchKernelGGL(fm_dft_lines_kernel, ge, blk, 0, st, h->d_fw2, h->d_fw0, R, C, C, 1, +1, h->d_wcR, h->d_wsR, n);   // inverse: columns, then rows
        hipLaunchKernelGGL(fm_dft_lines_kernel, ge, blk, 0, st, h->d_fw0, h->d_fw1, C, 1, R, C, +1, h->d_wcC, h->d_wsC, n);
        hipLaunchKernelGGL(fm_peak_kernel, dim3((unsigned)J), blk, 0, st, h->d_fw1, R, C, h->d_fres);
    };
    auto logpolar = [&](const float *img, float *lp) {
        dft2(img, h->d_fw0, h->d_fw1);
        hipLaunchKernelGGL(fm_mag_highpass_kernel, ge, blk, 0, st, h->d_fw0, h->d_hp, R, C, h->d_ff);
        hipLaunchKernelGGL(fm_remap_kernel, ge, blk, 0, st, h->d_ff, h->d_lpmap, R, C, lp);
    };
    logpolar(h->d_fa0, h->d_flp0);
    logpolar(h->d_fa1, h->d_flp1);
    phase_correlate(h->d_flp1, h->d_flp0);
    SCL_HIP(h, hipGetLastError());
    std::vector<double2> res((size_t)J);
    SCL_HIP(h, hipMemcpyAsync(res.data(), h->d_fres, sizeof(double2) * (size_t)J, hipMemcpyDeviceToHost, st));
    SCL_HIP(h, hipStreamSynchronize(st));
    // rotation and scale -> the inverted affine map of warpAffine (D.h:884-912; the expressions of iriso_fft_match)
    std::vector<double> mats((size_t)J * 6);
    std::vector<int> ok((size_t)J, 1);
    for (int j = 0; j < J; ++j) {
        const double rx = res[(size_t)j].x, ry = res[(size_t)j].y;
        float angle = (float)(180.0 * ry / (double)R);
        float scale = (float)std::pow((double)h->log_base, rx);
        if (scale > 1.8f) {
            angle = (float)(-180.0 * ry / (double)R);
            scale = (float)(1.0 / std::pow((double)h->log_base, rx));
            if (scale > 1.8f) ok[(size_t)j] = 0;
        }
        if (angle < -90.0f) angle += 180.0f; else if (angle > 90.0f) angle -= 180.0f;
        const double ang = (double)angle * M_PI / 180.0, sc = 1.0 / (double)scale;
        const double alpha = std::cos(ang) * sc, beta = std::sin(ang) * sc, pcx = (double)(float)(C / 2), pcy = (double)(float)(R / 2);
        double M[6] = {alpha, beta, (1.0 - alpha) * pcx - beta * pcy, -beta, alpha, beta * pcx + (1.0 - alpha) * pcy};
        double D = M[0] * M[4] - M[1] * M[3];
        D = D != 0.0 ? 1.0 / D : 0.0;
        const double A11 = M[4] * D, A22 = M[0] * D;
        M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
        const double b1 = -M[0] * M[2] - M[1] * M[5], b2 = -M[3] * M[2] - M[4] * M[5];
        M[2] = b1; M[5] = b2;
        for (int k = 0; k < 6; ++k) mats[(size_t)j * 6 + k] = M[k];
    }
    SCL_HIP(h, hipMemcpyAsync(h->d_fmats, mats.data(), sizeof(double) * mats.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(fm_warp_kernel, ge, blk, 0, st, h->d_fa1, h->d_fmats, R, C, h->d_frs);
    phase_correlate(h->d_frs, h->d_fa0);
    SCL_HIP(h, hipGetLastError());
    SCL_HIP(h, hipMemcpyAsync(res.data(), h->d_fres, sizeof(double2) * (size_t)J, hipMemcpyDeviceToHost, st));
    SCL_HIP(h, hipStreamSynchronize(st));
    for (int j = 0; j < J; ++j) {
        center_x[j] = ok[(size_t)j] ? (float)(res[(size_t)j].x + (double)(C / 2)) : 0.0f;
        if (ok_out) ok_out[j] = ok[(size_t)j];
    }
    return SCL_OK;
}

// compare(cur, candidate) for m candidates (D.h:964-1024): the FFT estimate(s), then the Hamming windows of five shifts around
// them -- the first pass against the candidate as it is, the second against the candidate turned by 180 columns -- as match_num says
int compare_jobs_locked(scl_iris *h, int cur, const int *cand, int m, float *dis, int *bias)
{
    const int mn = h->cfg.match_num, C = h->cfg.cols;
    const bool first = mn == 2 || mn == 0, second = mn == 2 || mn == 1;
    std::vector<FftJob> jobs;
    for (int c = 0; c < m; ++c) {
        if (first) jobs.push_back(FftJob{cand[c], 0, cur});
        if (second) jobs.push_back(FftJob{cand[c], 180, cur});                     // circShift(img2.img, 0, 180), D.h:978
    }
    std::vector<float> cx(jobs.size());
    int rc = fft_match_jobs_locked(h, jobs.data(), (int)jobs.size(), cx.data(), nullptr);
    if (rc) return rc;
    const int per = 5, J = (int)jobs.size();
    std::vector<int> jc((size_t)J), jr((size_t)J), shifts((size_t)J * per), jb((size_t)J);
    std::vector<float> jd((size_t)J);
    for (int j = 0; j < J; ++j) {
        jc[(size_t)j] = jobs[(size_t)j].key0; jr[(size_t)j] = jobs[(size_t)j].roll0;
        const int est = (int)(cx[(size_t)j] - (float)(C / 2));                     // int = float - int, D.h:969 / 980
        for (int t = 0; t < per; ++t) shifts[(size_t)j * per + t] = est - 2 + t;   // D.h:937
    }
    rc = hamming_jobs_locked(h, cur, jc.data(), shifts.data(), J, per, jd.data(), jb.data(), true, jr.data());
    if (rc) return rc;
    int j = 0;
    for (int c = 0; c < m; ++c) {
        float d1 = NAN, d2 = 0.0f; int b1 = -1, b2 = 0;
        if (first) { d1 = jd[(size_t)j]; b1 = jb[(size_t)j]; ++j; }
        if (second) { d2 = jd[(size_t)j]; b2 = jb[(size_t)j]; ++j; }
        if (mn == 2) { if (d1 < d2) { dis[c] = d1; bias[c] = b1; } else { dis[c] = d2; bias[c] = (b2 + 180) % 360; } }   // D.h:986-997
        else if (mn == 1) { dis[c] = d2; bias[c] = (b2 + 180) % 360; }
        else { dis[c] = d1; bias[c] = b1; }
    }
    return SCL_OK;
}

// Candidate search + pairwise comparison shared by the two detections (D.h:1100-1137 / 1205-1242).  `list` = global keys of
// the search set in the order the reference concatenates them (the KD-tree's point order); `cur` = global key of the query.
// Returns the position in `list` of the best candidate (-1: none), its distance and shift.
int detect_core_locked(scl_iris *h, int cur, const std::vector<int> &list, int *best_pos, float *best_dis, int *best_bias)
{
    *best_pos = -1; *best_dis = 10000000.0f; *best_bias = 0;                  // D.h:1104-1106
    const int n = (int)list.size(), k = h->cfg.num_candidates;
    if (n <= 0 || k <= 0) return SCL_OK;
    if ((size_t)n > h->list_cap) {
        h->list_cap = 0;
        const size_t cap = (size_t)n + (size_t)n / 2 + 256;
        int rc;
        if ((rc = dev_regrow(h, &h->d_list, cap)) || (rc = dev_regrow(h, &h->d_d2, cap))) return rc;
        h->list_cap = cap;
    }
    SCL_HIP(h, hipMemcpyAsync(h->d_list, list.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(iris_rowkey_d2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d_rowkeys, h->cfg.rows, cur, h->d_list, n, h->d_d2);
    SCL_HIP(h, hipGetLastError());
    std::vector<float> d2((size_t)n);
    SCL_HIP(h, hipMemcpyAsync(d2.data(), h->d_d2, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    // the k nearest: ascending distance, equal distances by ascending position; libnabo without ALLOW_SELF_MATCH skips
    // d2 <= eps; NaN / inf never enter (insertion like the engine's ring-key search)
    std::vector<int> pos; std::vector<float> pd;
    pos.reserve((size_t)k + 1); pd.reserve((size_t)k + 1);
    const float eps = h->cfg.knn_exclude_eps;
    for (int i = 0; i < n; ++i) {
        const float d = d2[(size_t)i];
        if (eps > 0.0f && d <= eps) continue;
        if (!(d < FLT_MAX)) continue;
        if ((int)pos.size() == k && !(d < pd.back())) continue;
        size_t j = pos.size();
        while (j > 0 && pd[j - 1] > d) --j;
        pos.insert(pos.begin() + (long)j, i); pd.insert(pd.begin() + (long)j, d);
        if ((int)pos.size() > k) { pos.pop_back(); pd.pop_back(); }
    }
    if (pos.empty()) return SCL_OK;
    const int m = (int)pos.size(), N = h->cfg.cols;
    std::vector<int> cand((size_t)m), bias((size_t)m);
    std::vector<float> dis((size_t)m);
    for (int c = 0; c < m; ++c) cand[(size_t)c] = list[(size_t)pos[(size_t)c]];
    int rc;
    if (h->cfg.shift_search == 1) {                                          // every column shift (a superset of compare()'s windows)
        std::vector<int> shifts((size_t)m * N);
        for (int c = 0; c < m; ++c) for (int j = 0; j < N; ++j) shifts[(size_t)c * N + j] = j;
        rc = hamming_jobs_locked(h, cur, cand.data(), shifts.data(), m, N, dis.data(), bias.data(), false);
    } else {
        rc = compare_jobs_locked(h, cur, cand.data(), m, dis.data(), bias.data());   // compare(), D.h:964-1024
    }
    if (rc) return rc;
    for (int c = 0; c < m; ++c)                                              // D.h:1112-1131: strict <, NaN never wins
        if (dis[(size_t)c] < *best_dis) { *best_dis = dis[(size_t)c]; *best_pos = pos[(size_t)c]; *best_bias = bias[(size_t)c]; }
    return SCL_OK;
}


// ---- the batch forms: host side ------------------------------------------------------------------------------------------------
int reserve(scl_iris *h, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return SCL_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
    const size_t cap = bytes + bytes / 4 + 256;
    SCL_HIP(h, hipMalloc(&b.p, cap));
    b.cap = cap;
    return SCL_OK;
}

// templates of the keyframes in slots slot0 .. slot0 + count - 1 from their stored images
int encode_slots_locked(scl_iris *h, int slot0, int count)
{
    const int rows = h->cfg.rows, cols = h->cfg.cols, pitch = (cols + 3) & ~3;
    int chunk_rows = kEncodeStageBytes / pitch;
    chunk_rows = chunk_rows < 1 ? 1 : (chunk_rows > rows ? rows : chunk_rows);
    const size_t lds = sizeof(unsigned int) * (2 * (size_t)h->words + (size_t)chunk_rows * (pitch / 4));
    for (int s = 0; s < count; s += 16384) {
        const int G = std::min(16384, count - s);
        hipLaunchKernelGGL(iris_encode_many_kernel, dim3((unsigned)cols, (unsigned)G), dim3(256), lds, h->stream, h->d_images, h->d_h, rows, cols,
                           h->cfg.nscale, h->d_T, h->d_M, h->words, slot0 + s, chunk_rows);
    }
    SCL_HIP(h, hipGetLastError());
    return SCL_OK;
}

// make_and_save for `count` scans: everything validated first, the database grown once, then launch groups of kIrisMaxGroup scans
// -- clouds to the device (neighbours in host memory in one transfer), one image launch over the group's points, one finishing
// launch into the slots, one encode launch -- and ONE wait for the device at the end, behind the copies for out_values
int make_and_save_many_locked(scl_iris *h, const void *const *clouds, const int *n_points, int stride, const int8_t *robots, const int *indexs,
                              int count, float *out_values)
{
    if (count < 0 || (count > 0 && (!clouds || !n_points || !robots || !indexs))) return fail(h, SCL_ERR_INVALID_ARG, "make_and_save_many: null array");
    for (int i = 0; i < count; ++i) {
        if (n_points[i] < 0 || stride < 12 || (stride & 3) || (n_points[i] > 0 && !clouds[i])) return fail(h, SCL_ERR_INVALID_ARG, "bad point layout");
        if (int rc = check_robot(h, robots[i], SCL_ERR_INVALID_ARG)) return rc;
    }
    if (count == 0) return SCL_OK;
    int rc = grow(h, h->reg.n + count);
    if (rc) return rc;
    const int rows = h->cfg.rows, cols = h->cfg.cols, slot0 = h->reg.n;
    const size_t cells = (size_t)rows * cols;
    // where every scan's points start in its group's buffer, and how many there are: one table for the call
    std::vector<unsigned long long> offs((size_t)count);
    size_t group_bytes = 0;
    for (int s = 0; s < count; s += kIrisMaxGroup) {
        size_t at = 0;
        for (int i = s; i < std::min(count, s + kIrisMaxGroup); ++i) { offs[(size_t)i] = at; at += (size_t)n_points[i] * stride; }
        group_bytes = std::max(group_bytes, at);
    }
    const int gmax = std::min(count, kIrisMaxGroup);
    if ((rc = reserve(h, h->bw.points, group_bytes)) || (rc = reserve(h, h->bw.planes, 2 * sizeof(int) * cells * gmax)) ||
        (rc = reserve(h, h->bw.table, (sizeof(unsigned long long) + sizeof(int)) * (size_t)count))) return rc;
    unsigned long long *d_offs = h->bw.table.as<unsigned long long>();
    int *d_counts = reinterpret_cast<int *>(d_offs + count);
    SCL_HIP(h, hipMemcpyAsync(d_offs, offs.data(), sizeof(unsigned long long) * (size_t)count, hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemcpyAsync(d_counts, n_points, sizeof(int) * (size_t)count, hipMemcpyHostToDevice, h->stream));
    unsigned char *d_pts = h->bw.points.as<unsigned char>();
    const bool beams_ok = h->cfg.nscan == 16 || h->cfg.nscan == 64;            // D.h:538 / 560: other beam counts leave the image empty
    for (int s = 0; s < count; s += kIrisMaxGroup) {
        const int G = std::min(kIrisMaxGroup, count - s);
        unsigned int *d_cells = h->bw.planes.as<unsigned int>();
        int *d_zmax = reinterpret_cast<int *>(d_cells + cells * G);
        int nmax = 0;
        for (int i = s; i < s + G;) {                                          // a run of clouds that lie back to back: one transfer
            const unsigned char *p0 = static_cast<const unsigned char *>(clouds[i]);
            size_t bytes = (size_t)n_points[i] * stride;
            int e = i + 1;
            while (e < s + G && (n_points[e] == 0 || (bytes > 0 && static_cast<const unsigned char *>(clouds[e]) == p0 + bytes))) { bytes += (size_t)n_points[e] * stride; ++e; }
            if (bytes) SCL_HIP(h, hipMemcpyAsync(d_pts + offs[(size_t)i], p0, bytes, hipMemcpyHostToDevice, h->stream));
            for (; i < e; ++i) nmax = std::max(nmax, n_points[i]);
        }
        SCL_HIP(h, hipMemsetAsync(d_cells, 0, 2 * sizeof(int) * cells * G, h->stream));
        if (nmax > 0 && beams_ok) {
            int blocks = (nmax + 255) / 256; blocks = blocks > 2048 ? 2048 : blocks;
            hipLaunchKernelGGL(iris_image_many_kernel, dim3((unsigned)blocks, (unsigned)G), dim3(256), 0, h->stream, d_pts, d_offs + s, d_counts + s, stride,
                               rows, cols, h->cfg.nscan == 16 ? 15.0 : 24.9, d_cells, d_zmax);
        }
        hipLaunchKernelGGL(iris_finish_many_kernel, dim3((unsigned)rows, (unsigned)G), dim3(128), sizeof(float) * cols, h->stream, d_zmax, d_cells, rows, cols,
                           slot0 + s, h->d_rowkeys, h->d_images);
        SCL_HIP(h, hipGetLastError());
        if ((rc = encode_slots_locked(h, slot0 + s, G))) return rc;
    }
    std::vector<unsigned char> img;
    std::vector<float> keys;
    if (out_values) {                                                          // D.h:1067-1081: image values row-major, then the row key
        img.resize(cells * count); keys.resize((size_t)rows * count);
        SCL_HIP(h, hipMemcpyAsync(img.data(), h->d_images + cells * slot0, cells * count, hipMemcpyDeviceToHost, h->stream));
        SCL_HIP(h, hipMemcpyAsync(keys.data(), h->d_rowkeys + (size_t)rows * slot0, sizeof(float) * rows * count, hipMemcpyDeviceToHost, h->stream));
    }
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    if (out_values)
        for (int i = 0; i < count; ++i) {
            float *o = out_values + (size_t)i * (cells + rows);
            for (size_t c = 0; c < cells; ++c) o[c] = (float)img[(size_t)i * cells + c];
            std::memcpy(o + cells, keys.data() + (size_t)i * rows, sizeof(float) * rows);
        }
    for (int i = 0; i < count; ++i) h->reg.commit(robots[i], indexs[i]);
    return SCL_OK;
}

// save_from_wire for `count` vectors: robot ids validated, the database grown once, one transfer, decode and encode on the device
int save_from_wire_many_locked(scl_iris *h, const float *values, const int8_t *robots, const int *indexs, int count)
{
    if (count < 0 || (count > 0 && (!values || !robots || !indexs))) return fail(h, SCL_ERR_INVALID_ARG, "save_from_wire_many: null array");
    for (int i = 0; i < count; ++i)
        if (int rc = check_robot(h, robots[i], SCL_ERR_INVALID_ARG)) return rc;
    if (count == 0) return SCL_OK;
    int rc = grow(h, h->reg.n + count);
    if (rc) return rc;
    const int rows = h->cfg.rows, cols = h->cfg.cols, slot0 = h->reg.n;
    const size_t per = (size_t)rows * cols + rows;
    if ((rc = reserve(h, h->bw.wire, sizeof(float) * per * count))) return rc;
    SCL_HIP(h, hipMemcpyAsync(h->bw.wire.p, values, sizeof(float) * per * count, hipMemcpyHostToDevice, h->stream));
    for (int s = 0; s < count; s += 16384) {
        const int G = std::min(16384, count - s);
        hipLaunchKernelGGL(iris_wire_decode_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)G), dim3(256), 0, h->stream,
                           h->bw.wire.as<float>() + per * s, rows, cols, h->cfg.wire_decode, slot0 + s, h->d_images, h->d_rowkeys);
    }
    SCL_HIP(h, hipGetLastError());
    if ((rc = encode_slots_locked(h, slot0, count))) return rc;
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < count; ++i) h->reg.commit(robots[i], indexs[i]);
    return SCL_OK;
}

// Work memory of the batched FFT shift estimate.  A job takes 72 bytes per pixel -- six float planes (both staged images, the
// highpassed magnitude, both log-polar images, the warped image) and three double2 planes -- 2.07 MB at 80 x 360, and a launch
// group of 16 queries x 10 candidates x 2 passes of compare() has 320 jobs: 664 MB.  One GiB holds that group in one pass (517 jobs
// at 80 x 360); a larger group, or a larger image, runs in ceil(jobs / (kIrisFftWorkBytes / (72 rows cols))) passes of two host
// visits each
constexpr size_t kIrisFftWorkBytes = (size_t)1 << 30;

// fft_match_jobs_locked for J jobs listed on the device (d_jobs; key0 < 0: an empty job): est[j] = (int)(center_x - (float)(cols / 2)),
// compare()'s shift estimate (D.h:969 / 980), to `est` on the host and, with the copy queued on the stream, to d_est.  The caller
// keeps `est` alive until it has synchronised.  Per pass the two host visits of the single call, for the same reason: the rotation
// and scale go through the C library's pow / cos / sin
int fft_estimate_many_locked(scl_iris *h, const FftJob *d_jobs, int J, std::vector<int> &est, int *d_est)
{
    est.assign((size_t)J, 0);
    if (J <= 0) return SCL_OK;
    const int R = h->cfg.rows, C = h->cfg.cols;
    const size_t n = (size_t)R * C;
    size_t pass = kIrisFftWorkBytes / (72 * n);
    pass = pass < 1 ? 1 : (pass > (size_t)J ? (size_t)J : pass);
    int rc;
    if ((rc = reserve(h, h->bw.fm, 72 * n * pass)) || (rc = reserve(h, h->bw.fres, sizeof(double2) * pass)) || (rc = reserve(h, h->bw.fmats, sizeof(double) * 6 * pass))) return rc;
    double2 *w0 = h->bw.fm.as<double2>(), *w1 = w0 + n * pass, *w2 = w1 + n * pass, *d_res = h->bw.fres.as<double2>();
    float *a0 = reinterpret_cast<float *>(w2 + n * pass), *a1 = a0 + n * pass, *ff = a1 + n * pass, *lp0 = ff + n * pass, *lp1 = lp0 + n * pass, *rs = lp1 + n * pass;
    double *d_mats = h->bw.fmats.as<double>();
    hipStream_t st = h->stream;
    std::vector<double2> res(pass);
    std::vector<double> mats(pass * 6);
    std::vector<int> ok(pass);
    for (size_t j0 = 0; j0 < (size_t)J; j0 += pass) {
        const size_t Jp = std::min(pass, (size_t)J - j0);
        const dim3 ge((unsigned)((n + 255) / 256), (unsigned)Jp), blk(256);
        hipLaunchKernelGGL(fm_stage_many_kernel, ge, blk, 0, st, h->d_images, d_jobs + j0, R, C, a0, a1);
        auto dft2 = [&](const float *src, double2 *w_out, double2 *w_tmp) {
            hipLaunchKernelGGL(fm_to_complex_kernel, ge, blk, 0, st, src, w_tmp, (int)n);
            hipLaunchKernelGGL(fm_dft_lines_kernel, ge, blk, 0, st, w_tmp, w_out, C, 1, R, C, -1, h->d_wcC, h->d_wsC, n);
            hipLaunchKernelGGL(fm_dft_lines_kernel, ge, blk, 0, st, w_out, w_tmp, R, C, C, 1, -1, h->d_wcR, h->d_wsR, n);
            (void)hipMemcpyAsync(w_out, w_tmp, sizeof(double2) * n * Jp, hipMemcpyDeviceToDevice, st);
        };
        auto phase_correlate = [&](const float *s1, const float *s2) {
            dft2(s1, w0, w2);
            dft2(s2, w1, w2);
            hipLaunchKernelGGL(fm_crosspower_kernel, ge, blk, 0, st, w0, w1, w2, (int)n);
            hipLaunchKernelGGL(fm_dft_lines_kernel, ge, blk, 0, st, w2, w0, R, C, C, 1, +1, h->d_wcR, h->d_wsR, n);
            hipLaunchKernelGGL(fm_dft_lines_kernel, ge, blk, 0, st, w0, w1, C, 1, R, C, +1, h->d_wcC, h->d_wsC, n);
            hipLaunchKernelGGL(fm_peak_kernel, dim3((unsigned)Jp), blk, 0, st, w1, R, C, d_res);
        };
        auto logpolar = [&](const float *img, float *lp) {
            dft2(img, w0, w1);
            hipLaunchKernelGGL(fm_mag_highpass_kernel, ge, blk, 0, st, w0, h->d_hp, R, C, ff);
            hipLaunchKernelGGL(fm_remap_kernel, ge, blk, 0, st, ff, h->d_lpmap, R, C, lp);
        };
        logpolar(a0, lp0);
        logpolar(a1, lp1);
        phase_correlate(lp1, lp0);
        SCL_HIP(h, hipGetLastError());
        SCL_HIP(h, hipMemcpyAsync(res.data(), d_res, sizeof(double2) * Jp, hipMemcpyDeviceToHost, st));
        SCL_HIP(h, hipStreamSynchronize(st));
        for (size_t j = 0; j < Jp; ++j) {                                      // the expressions of fft_match_jobs_locked (D.h:884-912)
            const double rx = res[j].x, ry = res[j].y;
            float angle = (float)(180.0 * ry / (double)R);
            float scale = (float)std::pow((double)h->log_base, rx);
            ok[j] = 1;
            if (scale > 1.8f) {
                angle = (float)(-180.0 * ry / (double)R);
                scale = (float)(1.0 / std::pow((double)h->log_base, rx));
                if (scale > 1.8f) ok[j] = 0;
            }
            if (angle < -90.0f) angle += 180.0f; else if (angle > 90.0f) angle -= 180.0f;
            const double ang = (double)angle * M_PI / 180.0, sc = 1.0 / (double)scale;
            const double alpha = std::cos(ang) * sc, beta = std::sin(ang) * sc, pcx = (double)(float)(C / 2), pcy = (double)(float)(R / 2);
            double M[6] = {alpha, beta, (1.0 - alpha) * pcx - beta * pcy, -beta, alpha, beta * pcx + (1.0 - alpha) * pcy};
            double D = M[0] * M[4] - M[1] * M[3];
            D = D != 0.0 ? 1.0 / D : 0.0;
            const double A11 = M[4] * D, A22 = M[0] * D;
            M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
            const double b1 = -M[0] * M[2] - M[1] * M[5], b2 = -M[3] * M[2] - M[4] * M[5];
            M[2] = b1; M[5] = b2;
            for (int k = 0; k < 6; ++k) mats[j * 6 + k] = M[k];
        }
        SCL_HIP(h, hipMemcpyAsync(d_mats, mats.data(), sizeof(double) * 6 * Jp, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(fm_warp_kernel, ge, blk, 0, st, a1, d_mats, R, C, rs);
        phase_correlate(rs, a0);
        SCL_HIP(h, hipGetLastError());
        SCL_HIP(h, hipMemcpyAsync(res.data(), d_res, sizeof(double2) * Jp, hipMemcpyDeviceToHost, st));
        SCL_HIP(h, hipStreamSynchronize(st));
        for (size_t j = 0; j < Jp; ++j) {
            const float center_x = ok[j] ? (float)(res[j].x + (double)(C / 2)) : 0.0f;
            est[j0 + j] = (int)(center_x - (float)(C / 2));                    // int = float - int, D.h:969 / 980
        }
    }
    SCL_HIP(h, hipMemcpyAsync(d_est, est.data(), sizeof(int) * (size_t)J, hipMemcpyHostToDevice, st));
    return SCL_OK;
}

// a query of a batched detection: keyframe `key` against the prefix [0, limit) of lists[which]; limit < 0: no search (the early-outs
// of the single calls, D.h:1092-1095 / 1198-1201), the query takes part in no launch
struct ManyQuery { int key, which, limit; };

// detect_core_locked for `count` queries.  The searching queries are ordered by list and cut into launch groups of kIrisDetectGroup;
// per group: row-key distances (one launch per list the group reaches), the selection, the job list, the Hamming matching -- every
// column shift, or the FFT estimate and the windows -- and the finishing kernel, all on the device; then one copy back and one wait
// (plus fft_estimate_many_locked's visits).  out[i] = (position in the list, shift, distance), (-1, 0, 10000000) where nothing was
// searched or found
int detect_many_locked(scl_iris *h, const std::vector<ManyQuery> &qs, const std::vector<int> lists[2], std::vector<IrisAnswer> &out)
{
    const int count = (int)qs.size(), k = h->cfg.num_candidates, N = h->cfg.cols, rows = h->cfg.rows;
    out.assign((size_t)count, IrisAnswer{-1, 0, 10000000.0f});
    std::vector<int> order;
    int used[2] = {0, 0};
    for (int l = 0; l < 2; ++l)
        for (int i = 0; i < count; ++i)
            if (qs[(size_t)i].limit > 0 && qs[(size_t)i].which == l) { order.push_back(i); used[l] = std::max(used[l], qs[(size_t)i].limit); }
    const int nact = (int)order.size();
    if (nact == 0) return SCL_OK;
    const bool window = h->cfg.shift_search != 1;
    const int mn = h->cfg.match_num, passes = window ? (mn == 2 ? 2 : 1) : 0, per = window ? 5 : N;
    const int off[2] = {0, used[0]};
    int rc;
    if ((rc = reserve(h, h->bw.list, sizeof(int) * ((size_t)used[0] + used[1]))) || (rc = reserve(h, h->bw.query, sizeof(int) * 3 * (size_t)nact)) ||
        (rc = reserve(h, h->bw.answers, sizeof(IrisAnswer) * (size_t)nact))) return rc;
    std::vector<int> hq(3 * (size_t)nact);                                     // key | limit | list offset
    for (int j = 0; j < nact; ++j) {
        const ManyQuery &q = qs[(size_t)order[(size_t)j]];
        hq[(size_t)j] = q.key; hq[(size_t)nact + j] = q.limit; hq[2 * (size_t)nact + j] = off[q.which];
    }
    int *d_list = h->bw.list.as<int>(), *d_qkey = h->bw.query.as<int>(), *d_limit = d_qkey + nact, *d_off = d_limit + nact;
    IrisAnswer *d_ans = h->bw.answers.as<IrisAnswer>();
    for (int l = 0; l < 2; ++l)
        if (used[l] > 0) SCL_HIP(h, hipMemcpyAsync(d_list + off[l], lists[l].data(), sizeof(int) * (size_t)used[l], hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemcpyAsync(d_qkey, hq.data(), sizeof(int) * hq.size(), hipMemcpyHostToDevice, h->stream));
    const size_t fw = (size_t)N * h->words;
    std::vector<IrisAnswer> ans((size_t)nact);
    std::vector<int> est, cpos;
    for (int s = 0; s < nact; s += kIrisDetectGroup) {
        const int G = std::min(kIrisDetectGroup, nact - s);
        int nmax = 0;
        for (int j = s; j < s + G; ++j) nmax = std::max(nmax, hq[(size_t)nact + j]);
        const int m = std::min(k, nmax);                                       // candidate slots per query: no more can qualify
        const size_t slots = (size_t)G * m, J = slots * (window ? passes : 1);
        if ((rc = reserve(h, h->bw.d2, sizeof(float) * (size_t)G * nmax)) || (rc = reserve(h, h->bw.cand, sizeof(int) * 2 * slots)) ||
            (rc = reserve(h, h->bw.jobs, sizeof(FftJob) * J)) || (rc = reserve(h, h->bw.est, sizeof(int) * J)) ||
            (rc = reserve(h, h->bw.counts, sizeof(int) * 2 * J * per))) return rc;
        float *d_d2 = h->bw.d2.as<float>();
        int *d_cpos = h->bw.cand.as<int>(), *d_ckey = d_cpos + slots, *d_est = h->bw.est.as<int>();
        int *d_diff = h->bw.counts.as<int>(), *d_total = d_diff + J * per;
        FftJob *d_jobs = h->bw.jobs.as<FftJob>();
        for (int a = s; a < s + G;) {                                          // the group's queries of one list: one launch
            int b = a, n = 0;
            while (b < s + G && hq[2 * (size_t)nact + b] == hq[2 * (size_t)nact + a]) { n = std::max(n, hq[(size_t)nact + b]); ++b; }
            hipLaunchKernelGGL(iris_rowkey_d2_many_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), sizeof(float) * kIrisDetectGroup * rows, h->stream,
                               h->d_rowkeys, rows, d_qkey + a, d_limit + a, b - a, d_list + hq[2 * (size_t)nact + a], n, d_d2 + (size_t)(a - s) * nmax, nmax);
            a = b;
        }
        hipLaunchKernelGGL(iris_select_kernel, dim3((unsigned)G), dim3(256), 0, h->stream, d_d2, nmax, d_limit + s, m, h->cfg.knn_exclude_eps, d_cpos);
        hipLaunchKernelGGL(iris_jobs_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, h->stream, d_cpos, d_qkey + s, d_off + s, d_list, G, m,
                           passes, mn == 1 ? 180 : 0, d_ckey, d_jobs);
        SCL_HIP(h, hipGetLastError());
        if (window && !h->fm_ok) {
            // the single call fails where a query has a candidate to compare (fft_match_jobs_locked with J > 0): so does the batch
            cpos.resize(slots);
            SCL_HIP(h, hipMemcpyAsync(cpos.data(), d_cpos, sizeof(int) * slots, hipMemcpyDeviceToHost, h->stream));
            SCL_HIP(h, hipStreamSynchronize(h->stream));
            for (int q = 0; q < G; ++q)
                if (cpos[(size_t)q * m] >= 0) return fail(h, SCL_ERR_UNSUPPORTED, "the FFT shift estimate takes even rows and columns only");
            for (int q = 0; q < G; ++q) ans[(size_t)s + q] = IrisAnswer{-1, 0, 10000000.0f};
            continue;
        }
        if (window) {
            if ((rc = fft_estimate_many_locked(h, d_jobs, (int)J, est, d_est))) return rc;
            hipLaunchKernelGGL(iris_hamming_window_kernel, dim3((unsigned)J), dim3(256), 0, h->stream, h->d_T, h->d_M, fw, d_jobs, d_est, N, h->words, h->trows,
                               d_diff, d_total);
        } else {
            hipLaunchKernelGGL(iris_hamming_all_many_kernel, dim3((unsigned)(slots * N)), dim3(64), 0, h->stream, h->d_T, h->d_M, fw, d_qkey + s, d_ckey, m, N,
                               h->words, h->trows, d_diff, d_total);
        }
        hipLaunchKernelGGL(iris_finish_detect_kernel, dim3(1), dim3(kIrisDetectGroup), 0, h->stream, d_cpos, d_est, d_diff, d_total, G, m, per, window ? 1 : 0,
                           window ? passes : 1, mn, d_ans + s);
        SCL_HIP(h, hipGetLastError());
        SCL_HIP(h, hipMemcpyAsync(ans.data() + s, d_ans + s, sizeof(IrisAnswer) * (size_t)G, hipMemcpyDeviceToHost, h->stream));
        SCL_HIP(h, hipStreamSynchronize(h->stream));
    }
    for (int j = 0; j < nact; ++j) out[(size_t)order[(size_t)j]] = ans[(size_t)j];
    return SCL_OK;
}

int detect_intra_many_locked(scl_iris *h, const int *curs, int count, int *loop_ids, float *biases, float *dists)
{
    const std::vector<int> &mine = h->reg.keys_of(h->cfg.this_id);
    for (int i = 0; i < count; ++i)
        if (curs[i] < 0 || curs[i] >= (int)mine.size()) return fail(h, SCL_ERR_OUT_OF_RANGE, "detect_intra: no such keyframe of this robot");
    std::vector<ManyQuery> qs((size_t)count);
    for (int i = 0; i < count; ++i) {
        const bool search = curs[i] >= h->cfg.num_exclude_recent + h->cfg.num_candidates + 1;      // D.h:1092-1095
        qs[(size_t)i] = ManyQuery{mine[(size_t)curs[i]], 0, search ? curs[i] - h->cfg.num_exclude_recent : -1};
    }
    const std::vector<int> lists[2] = {mine, std::vector<int>()};
    std::vector<IrisAnswer> ans;
    int rc = detect_many_locked(h, qs, lists, ans);
    if (rc) return rc;
    for (int i = 0; i < count; ++i) {
        const IrisAnswer &a = ans[(size_t)i];
        const bool loop = (double)a.dis < h->cfg.dist_thres;                   // D.h:1140-1144: the LOCAL index
        loop_ids[i] = loop ? a.pos : -1; biases[i] = loop ? (float)a.bias : 0.0f;
        if (dists) dists[i] = a.dis;
    }
    return SCL_OK;
}

int detect_inter_many_locked(scl_iris *h, const int *curs, int count, int *loop_ids, float *biases, float *dists)
{
    for (int i = 0; i < count; ++i)
        if (curs[i] < 0 || curs[i] >= h->reg.n) return fail(h, SCL_ERR_OUT_OF_RANGE, "detect_inter: key out of range");
    // a received keyframe searches this robot's keys (list 0), one of this robot every other robot's in the registry's
    // concatenation order, unsorted (list 1): KeyframeRegistry::inter_candidates
    std::vector<int> lists[2];
    lists[0] = h->reg.keys_of(h->cfg.this_id);
    for (int r = 0; r < h->reg.robot_num; ++r)
        if (r != h->cfg.this_id) lists[1].insert(lists[1].end(), h->reg.keys_of(r).begin(), h->reg.keys_of(r).end());
    std::vector<ManyQuery> qs((size_t)count);
    for (int i = 0; i < count; ++i) {
        const int which = h->reg.robots[(size_t)curs[i]] == h->cfg.this_id ? 1 : 0, n = (int)lists[which].size();
        qs[(size_t)i] = ManyQuery{curs[i], which, n >= h->cfg.num_candidates + 1 ? n : -1};          // D.h:1198-1201
    }
    std::vector<IrisAnswer> ans;
    int rc = detect_many_locked(h, qs, lists, ans);
    if (rc) return rc;
    for (int i = 0; i < count; ++i) {
        const IrisAnswer &a = ans[(size_t)i];
        const bool loop = (double)a.dis < h->cfg.dist_thres && a.pos >= 0;     // D.h:1236, 1245-1248: the GLOBAL key
        loop_ids[i] = loop ? lists[qs[(size_t)i].which][(size_t)a.pos] : -1; biases[i] = loop ? (float)a.bias : 0.0f;
        if (dists) dists[i] = a.dis;
    }
    return SCL_OK;
}

// The exhaustive ranked search for `count` queries (ManyQuery as in detect_many_locked; limit <= 0: an empty search set).  The
// searching queries are ordered by list and cut into launch groups of kIrisDetectGroup; per group the scoring launch (one per list
// the group reaches: every candidate below the group's longest prefix against every query of the group), iris_select_kernel over the
// scores -- k rounds over n floats per query, next to nothing beside n * cols * cols * words word steps of scoring, and the order
// (score bits, position) with NaN left out is the one it already implements -- and the finishing kernel; everything on the stream,
// ONE copy back and ONE wait for the whole call.  out[i * k + j]: rank j of query i, (-1, 0, +inf) from the first unused slot on
int search_many_locked(scl_iris *h, const std::vector<ManyQuery> &qs, const std::vector<int> lists[2], int k, std::vector<IrisSearchEntry> &out)
{
    const int count = (int)qs.size(), N = h->cfg.cols;
    out.assign((size_t)count * k, IrisSearchEntry{-1, 0, INFINITY});
    std::vector<int> order;
    int used[2] = {0, 0};
    for (int l = 0; l < 2; ++l)
        for (int i = 0; i < count; ++i)
            if (qs[(size_t)i].limit > 0 && qs[(size_t)i].which == l) { order.push_back(i); used[l] = std::max(used[l], qs[(size_t)i].limit); }
    const int nact = (int)order.size();
    if (nact == 0) return SCL_OK;
    const int off[2] = {0, used[0]}, nmax = std::max(used[0], used[1]);
    const size_t n_res = (size_t)nact * k;
    int rc;
    if ((rc = reserve(h, h->bw.list, sizeof(int) * ((size_t)used[0] + used[1]))) || (rc = reserve(h, h->bw.query, sizeof(int) * 3 * (size_t)nact)) ||
        (rc = reserve(h, h->bw.sscore, sizeof(float) * (size_t)kIrisDetectGroup * nmax)) || (rc = reserve(h, h->bw.sbias, sizeof(int) * (size_t)kIrisDetectGroup * nmax)) ||
        (rc = reserve(h, h->bw.spos, sizeof(int) * n_res)) || (rc = reserve(h, h->bw.sres, sizeof(IrisSearchEntry) * n_res))) return rc;
    std::vector<int> hq(3 * (size_t)nact);                                     // key | limit | list offset
    for (int j = 0; j < nact; ++j) {
        const ManyQuery &q = qs[(size_t)order[(size_t)j]];
        hq[(size_t)j] = q.key; hq[(size_t)nact + j] = q.limit; hq[2 * (size_t)nact + j] = off[q.which];
    }
    int *d_list = h->bw.list.as<int>(), *d_qkey = h->bw.query.as<int>(), *d_limit = d_qkey + nact;
    float *d_score = h->bw.sscore.as<float>();
    int *d_bias = h->bw.sbias.as<int>(), *d_pos = h->bw.spos.as<int>();
    IrisSearchEntry *d_res = h->bw.sres.as<IrisSearchEntry>();
    for (int l = 0; l < 2; ++l)
        if (used[l] > 0) SCL_HIP(h, hipMemcpyAsync(d_list + off[l], lists[l].data(), sizeof(int) * (size_t)used[l], hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemcpyAsync(d_qkey, hq.data(), sizeof(int) * hq.size(), hipMemcpyHostToDevice, h->stream));
    const size_t fw = (size_t)N * h->words, lds = sizeof(uint2) * (size_t)N * (size_t)(h->words | 1);
    const int threads = std::min(kSearchMaxThreads, (N + 63) / 64 * 64);
    for (int s = 0; s < nact; s += kIrisDetectGroup) {
        const int G = std::min(kIrisDetectGroup, nact - s);
        for (int a = s; a < s + G;) {                                          // the group's queries of one list: one launch
            int b = a, n = 0;
            while (b < s + G && hq[2 * (size_t)nact + b] == hq[2 * (size_t)nact + a]) { n = std::max(n, hq[(size_t)nact + b]); ++b; }
            float *sc = d_score + (size_t)(a - s) * nmax;
            int *bi = d_bias + (size_t)(a - s) * nmax;
            if (lds <= kSearchLdsBytes)
                hipLaunchKernelGGL(iris_search_score_kernel<true>, dim3((unsigned)n), dim3((unsigned)threads), lds, h->stream, h->d_T, h->d_M, fw, d_qkey + a,
                                   d_limit + a, b - a, d_list + hq[2 * (size_t)nact + a], N, h->words, h->trows, sc, bi, nmax);
            else
                hipLaunchKernelGGL(iris_search_score_kernel<false>, dim3((unsigned)n), dim3((unsigned)threads), 0, h->stream, h->d_T, h->d_M, fw, d_qkey + a,
                                   d_limit + a, b - a, d_list + hq[2 * (size_t)nact + a], N, h->words, h->trows, sc, bi, nmax);
            a = b;
        }
        hipLaunchKernelGGL(iris_select_kernel, dim3((unsigned)G), dim3(256), 0, h->stream, d_score, nmax, d_limit + s, k, 0.0f, d_pos + (size_t)s * k);
        hipLaunchKernelGGL(iris_search_finish_kernel, dim3((unsigned)((G * k + 255) / 256)), dim3(256), 0, h->stream, d_pos + (size_t)s * k, d_score, d_bias, nmax, G, k,
                           d_res + (size_t)s * k);
        SCL_HIP(h, hipGetLastError());
    }
    std::vector<IrisSearchEntry> res(n_res);
    SCL_HIP(h, hipMemcpyAsync(res.data(), d_res, sizeof(IrisSearchEntry) * n_res, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    for (int j = 0; j < nact; ++j) std::copy_n(res.begin() + (size_t)j * k, k, out.begin() + (size_t)order[(size_t)j] * k);
    return SCL_OK;
}

// the lists from the entries: the listed candidates first, then (-1, 0, +inf) up to k; to_id: position in the query's list -> id
template <class ToId>
void report_search(const std::vector<IrisSearchEntry> &res, int count, int k, ToId to_id, int *cand_ids, float *cand_biases, float *cand_dists, int *n_found)
{
    for (int i = 0; i < count; ++i) {
        int found = 0;
        for (int j = 0; j < k; ++j) {
            const IrisSearchEntry &e = res[(size_t)i * k + j];
            found += e.pos >= 0;
            cand_ids[(size_t)i * k + j] = e.pos >= 0 ? to_id(i, e.pos) : -1;
            if (cand_biases) cand_biases[(size_t)i * k + j] = (float)e.bias;
            if (cand_dists) cand_dists[(size_t)i * k + j] = e.dis;
        }
        if (n_found) n_found[i] = found;
    }
}

inline bool search_k_ok(int k) { return k >= 1 && k <= SCL_IRIS_SEARCH_MAX; }

int search_intra_locked(scl_iris *h, const int *curs, int count, int k, int *cand_ids, float *cand_biases, float *cand_dists, int *n_found)
{
    if (!search_k_ok(k)) return fail(h, SCL_ERR_INVALID_ARG, "search_intra: k outside [1, SCL_IRIS_SEARCH_MAX]");
    const std::vector<int> &mine = h->reg.keys_of(h->cfg.this_id);
    for (int i = 0; i < count; ++i)
        if (curs[i] < 0 || curs[i] >= (int)mine.size()) return fail(h, SCL_ERR_OUT_OF_RANGE, "search_intra: no such keyframe of this robot");
    if (count == 0) return SCL_OK;
    std::vector<ManyQuery> qs((size_t)count);
    for (int i = 0; i < count; ++i) qs[(size_t)i] = ManyQuery{mine[(size_t)curs[i]], 0, curs[i] - h->cfg.num_exclude_recent};
    const std::vector<int> lists[2] = {mine, std::vector<int>()};
    std::vector<IrisSearchEntry> res;
    int rc = search_many_locked(h, qs, lists, k, res);
    if (rc) return rc;
    report_search(res, count, k, [](int, int pos) { return pos; }, cand_ids, cand_biases, cand_dists, n_found);     // the LOCAL index
    return SCL_OK;
}

int search_inter_locked(scl_iris *h, const int *curs, int count, int k, int *cand_ids, float *cand_biases, float *cand_dists, int *n_found)
{
    if (!search_k_ok(k)) return fail(h, SCL_ERR_INVALID_ARG, "search_inter: k outside [1, SCL_IRIS_SEARCH_MAX]");
    for (int i = 0; i < count; ++i)
        if (curs[i] < 0 || curs[i] >= h->reg.n) return fail(h, SCL_ERR_OUT_OF_RANGE, "search_inter: key out of range");
    if (count == 0) return SCL_OK;
    std::vector<int> lists[2];                                                 // the lists of detect_inter_many_locked
    lists[0] = h->reg.keys_of(h->cfg.this_id);
    for (int r = 0; r < h->reg.robot_num; ++r)
        if (r != h->cfg.this_id) lists[1].insert(lists[1].end(), h->reg.keys_of(r).begin(), h->reg.keys_of(r).end());
    std::vector<ManyQuery> qs((size_t)count);
    for (int i = 0; i < count; ++i) {
        const int which = h->reg.robots[(size_t)curs[i]] == h->cfg.this_id ? 1 : 0;
        qs[(size_t)i] = ManyQuery{curs[i], which, (int)lists[which].size()};
    }
    std::vector<IrisSearchEntry> res;
    int rc = search_many_locked(h, qs, lists, k, res);
    if (rc) return rc;
    report_search(res, count, k, [&](int i, int pos) { return lists[qs[(size_t)i].which][(size_t)pos]; }, cand_ids, cand_biases, cand_dists, n_found);   // the GLOBAL key
    return SCL_OK;
}

}  // namespace

extern "C" {

int scl_iris_default_config(scl_iris_config *c)
{
    if (!c) return SCL_ERR_INVALID_ARG;
    c->rows = 80; c->cols = 360; c->nscan = 64; c->nscale = 4; c->min_wavelength = 18; c->mult = 1.6f; c->sigma_onf = 0.75f; c->device = 0;
    c->dist_thres = 0.32; c->num_exclude_recent = 30; c->match_num = 2; c->num_candidates = 10; c->robot_num = 1; c->this_id = 0;
    c->knn_exclude_eps = FLT_EPSILON; c->wire_decode = 0; c->shift_search = 0;
    return SCL_OK;
}

const char *scl_iris_last_error(const scl_iris *h) { return h ? h->last_error.c_str() : "null handle"; }

int scl_iris_create(const scl_iris_config *cfg, scl_iris **out)
{
    if (!cfg || !out) return SCL_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->rows < 1 || cfg->rows > 512 || cfg->cols < 1 || cfg->cols > 2048 || cfg->nscale < 1 || cfg->nscale > 8 ||
        cfg->min_wavelength < 1 || !(cfg->mult > 0.f) || !(cfg->sigma_onf > 0.f) || cfg->sigma_onf == 1.0f ||
        cfg->robot_num < 1 || cfg->robot_num > 127 || cfg->this_id < 0 || cfg->this_id >= cfg->robot_num || cfg->num_candidates < 1 ||
        cfg->num_candidates > 4096 || cfg->num_exclude_recent < 0 || cfg->match_num < 0 || cfg->match_num > 2 || !(cfg->knn_exclude_eps >= 0.0f) ||
        cfg->shift_search < 0 || cfg->shift_search > 1)
        return SCL_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SCL_ERR_NO_DEVICE;
    if (cfg->device < 0 || cfg->device >= ndev) return SCL_ERR_INVALID_ARG;
    scl_iris *h = new (std::nothrow) scl_iris();
    if (!h) return SCL_ERR_NOMEM;
    h->cfg = *cfg; h->device = cfg->device;
    h->reg.init(cfg->robot_num);                                                // D.h:501-509
    h->trows = 2 * cfg->nscale * cfg->rows; h->words = (h->trows + 31) / 32;
    auto bail = [&](int code) { scl_iris_destroy(h); return code; };
    if (hipSetDevice(h->device) != hipSuccess) return bail(SCL_ERR_HIP);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return bail(SCL_ERR_HIP);
    const size_t cells = (size_t)cfg->rows * cfg->cols;
    int rc;
    if ((rc = dev_alloc(h, &h->d_cells, cells)) || (rc = dev_alloc(h, &h->d_zmax, cells)) || (rc = dev_alloc(h, &h->d_img1, cells)) ||
        (rc = dev_alloc(h, &h->d_key1, (size_t)cfg->rows)) || (rc = dev_alloc(h, &h->d_h, (size_t)cfg->nscale * cfg->cols)) ||
        (rc = dev_alloc(h, &h->d_unpack, (size_t)h->trows * cfg->cols))) return bail(rc);
    // the one-sided log-Gabor transfer functions, D.h:622-640 (float arithmetic like cv::log / pow / exp on Mat1f)
    const int N = cfg->cols, ndata = N - (N & 1);
    std::vector<float> g((size_t)cfg->nscale * N, 0.0f);
    double wavelength = cfg->min_wavelength;
    for (int s = 0; s < cfg->nscale; ++s) {
        const double fo = 1.0 / wavelength;
        for (int i = 0; i < ndata / 2 + 1; ++i) {
            const float radius = i == 0 ? 1.0f : (float)i / (float)ndata;
            float t = std::log((float)((double)radius / fo));
            t = t * t;
            const double denom = 2 * std::log((double)cfg->sigma_onf) * std::log((double)cfg->sigma_onf);
            g[(size_t)s * N + i] = std::exp((float)((double)(-t) / denom));
        }
        g[(size_t)s * N] = 0.0f;
        wavelength *= (double)cfg->mult;
    }
    // h[s][n] = sum_k G[k] e^{2 pi i k n / N} in fp64 on the host (once per engine; the CPU restatement forms the same sums
    // with the same libm, so the templates agree bit for bit)
    {
        const double TWO_PI = 6.283185307179586476925286766559;
        std::vector<double2> hh((size_t)cfg->nscale * N);
        for (int s = 0; s < cfg->nscale; ++s)
            for (int n = 0; n < N; ++n) {
                double re = 0.0, im = 0.0;
                for (int k = 0; k < N; ++k) {
                    const float gk = g[(size_t)s * N + k];
                    if (gk == 0.0f) continue;
                    const double a = TWO_PI * (double)(((long long)k * n) % N) / (double)N;
                    re += (double)gk * std::cos(a); im += (double)gk * std::sin(a);
                }
                hh[(size_t)s * N + n] = make_double2(re, im);
            }
        if (hipMemcpy(h->d_h, hh.data(), sizeof(double2) * hh.size(), hipMemcpyHostToDevice) != hipSuccess) return bail(SCL_ERR_HIP);
    }
    // tables of the FFT shift estimate (logPolarFFTTemplateMatch, D.h:719-925): the expressions of oracle/iris_oracle.c's
    // iriso_fft_match, evaluated here with the same C library -- twiddles, highpass, log-polar map in OpenCV's fixed point
    h->fm_ok = !(cfg->rows & 1) && !(cfg->cols & 1) && cfg->rows >= 6 && cfg->cols >= 6;
    if (h->fm_ok) {
        const int R = cfg->rows, C = cfg->cols;
        std::vector<double> wcR((size_t)R), wsR((size_t)R), wcC((size_t)C), wsC((size_t)C);
        for (int k = 0; k < R; ++k) { wcR[(size_t)k] = std::cos(2.0 * M_PI * (double)k / (double)R); wsR[(size_t)k] = std::sin(2.0 * M_PI * (double)k / (double)R); }
        for (int k = 0; k < C; ++k) { wcC[(size_t)k] = std::cos(2.0 * M_PI * (double)k / (double)C); wsC[(size_t)k] = std::sin(2.0 * M_PI * (double)k / (double)C); }
        std::vector<float> a((size_t)R), b((size_t)C), hp(cells);
        { const float step = (float)(M_PI / (double)R); float val = (float)(-M_PI * 0.5); for (int i = 0; i < R; ++i) { a[(size_t)i] = cosf(val); val += step; } }
        { const float step = (float)(M_PI / (double)C); float val = (float)(-M_PI * 0.5); for (int j = 0; j < C; ++j) { b[(size_t)j] = cosf(val); val += step; } }
        for (int i = 0; i < R; ++i)
            for (int j = 0; j < C; ++j) { const float t = a[(size_t)i] * b[(size_t)j]; hp[(size_t)i * C + j] = (1.0f - t) * (2.0f - t); }
        std::vector<int2> map(cells);
        const float radii = (float)C, angles = (float)R, cxf = (float)(C / 2), cyf = (float)(R / 2);
        const float ddx = (float)C - cxf, ddy = (float)R - cyf;
        const float d = (float)std::sqrt((double)ddx * (double)ddx + (double)ddy * (double)ddy);
        const float log_base = (float)std::pow(10.0, (double)(log10f(d) / radii));
        const float d_theta = (float)(M_PI / (double)angles);
        float theta = (float)(M_PI / 2.0);
        for (int i = 0; i < R; ++i) {
            for (int j = 0; j < C; ++j) {
                const float radius = powf(log_base, (float)j);
                const float x = radius * sinf(theta) + cxf, y = radius * cosf(theta) + cyf;
                map[(size_t)i * C + j] = make_int2((int)lrint((double)x * 32.0), (int)lrint((double)y * 32.0));
            }
            theta += d_theta;
        }
        h->log_base = log_base;
        if ((rc = dev_alloc(h, &h->d_wcR, (size_t)R)) || (rc = dev_alloc(h, &h->d_wsR, (size_t)R)) || (rc = dev_alloc(h, &h->d_wcC, (size_t)C)) || (rc = dev_alloc(h, &h->d_wsC, (size_t)C)) ||
            (rc = dev_alloc(h, &h->d_hp, cells)) || (rc = dev_alloc(h, &h->d_lpmap, cells))) return bail(rc);
        if (hipMemcpy(h->d_wcR, wcR.data(), sizeof(double) * R, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(h->d_wsR, wsR.data(), sizeof(double) * R, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_wcC, wcC.data(), sizeof(double) * C, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(h->d_wsC, wsC.data(), sizeof(double) * C, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_hp, hp.data(), sizeof(float) * cells, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(h->d_lpmap, map.data(), sizeof(int2) * cells, hipMemcpyHostToDevice) != hipSuccess)
            return bail(SCL_ERR_HIP);
    }
    *out = h;
    return SCL_OK;
}

int scl_iris_destroy(scl_iris *h)
{
    if (!h) return SCL_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void *p : {(void *)h->d_images, (void *)h->d_rowkeys, (void *)h->d_T, (void *)h->d_M, (void *)h->d_h, (void *)h->d_cells, (void *)h->d_zmax,
                    (void *)h->d_points, (void *)h->d_img1, (void *)h->d_key1, (void *)h->d_unpack, (void *)h->d_cand, (void *)h->d_shifts,
                    (void *)h->d_diff, (void *)h->d_total, (void *)h->d_list, (void *)h->d_d2, (void *)h->d_wcR, (void *)h->d_wsR, (void *)h->d_wcC, (void *)h->d_wsC,
                    (void *)h->d_hp, (void *)h->d_lpmap, (void *)h->d_fjobs, (void *)h->d_fa0, (void *)h->d_fa1, (void *)h->d_ff, (void *)h->d_flp0, (void *)h->d_flp1,
                    (void *)h->d_frs, (void *)h->d_fw0, (void *)h->d_fw1, (void *)h->d_fw2, (void *)h->d_fres, (void *)h->d_fmats, (void *)h->d_rolls})
        if (p) (void)hipFree(p);
    h->bw.release();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return SCL_OK;
}

int scl_iris_make_image(scl_iris *h, const void *points, int n_points, int stride_bytes, uint8_t *image, float *rowkey)
{
    if (!h || !image || !rowkey) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    int rc = make_image_locked(h, points, n_points, stride_bytes);
    if (rc) return rc;
    SCL_HIP(h, hipMemcpyAsync(image, h->d_img1, (size_t)h->cfg.rows * h->cfg.cols, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipMemcpyAsync(rowkey, h->d_key1, sizeof(float) * h->cfg.rows, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    return SCL_OK;
}

int scl_iris_make_and_save(scl_iris *h, const void *points, int n_points, int stride_bytes, int8_t robot, int index, float *out_values)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    int rc = make_image_locked(h, points, n_points, stride_bytes);
    if (rc) return rc;
    if ((rc = append_locked(h, robot, index))) return rc;
    if (out_values) {                                                         // D.h:1067-1081: image values row-major, then the row key
        const size_t cells = (size_t)h->cfg.rows * h->cfg.cols;
        std::vector<unsigned char> img(cells);
        SCL_HIP(h, hipMemcpyAsync(img.data(), h->d_img1, cells, hipMemcpyDeviceToHost, h->stream));
        SCL_HIP(h, hipMemcpyAsync(out_values + cells, h->d_key1, sizeof(float) * h->cfg.rows, hipMemcpyDeviceToHost, h->stream));
        SCL_HIP(h, hipStreamSynchronize(h->stream));
        for (size_t i = 0; i < cells; ++i) out_values[i] = (float)img[i];
    }
    return SCL_OK;
}

int scl_iris_save_image(scl_iris *h, const uint8_t *image, const float *rowkey, int8_t robot, int index)
{
    if (!h || !image || !rowkey) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    SCL_HIP(h, hipMemcpyAsync(h->d_img1, image, (size_t)h->cfg.rows * h->cfg.cols, hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemcpyAsync(h->d_key1, rowkey, sizeof(float) * h->cfg.rows, hipMemcpyHostToDevice, h->stream));
    return append_locked(h, robot, index);
}

int scl_iris_save_from_wire(scl_iris *h, const float *values, int8_t robot, int index)
{
    if (!h || !values) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    const int rows = h->cfg.rows, cols = h->cfg.cols;
    std::vector<uint8_t> img((size_t)rows * cols);
    auto to_u8 = [](float f) -> uint8_t {                                     // float -> uchar as x86 does it: cvttss2si, low byte
        if (!(f > -2147483904.0f && f < 2147483648.0f)) return 0;              // (out of int range / NaN -> 0x80000000 -> 0)
        return (uint8_t)(int32_t)f;
    };
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c)
            img[(size_t)r * cols + c] = to_u8(h->cfg.wire_decode ? values[(size_t)r * cols + c]             // D.h:1067-1074's layout
                                                               : values[(size_t)r * (cols + 1) + c + 1]);   // D.h:1035
    SCL_HIP(h, hipMemcpyAsync(h->d_img1, img.data(), img.size(), hipMemcpyHostToDevice, h->stream));
    SCL_HIP(h, hipMemcpyAsync(h->d_key1, values + (size_t)rows * cols, sizeof(float) * rows, hipMemcpyHostToDevice, h->stream));   // D.h:1039-1042
    return append_locked(h, robot, index);                                    // synchronises before `img` goes away
}

int scl_iris_get_size(const scl_iris *h) { return get_size(h); }
int scl_iris_get_size_of(const scl_iris *h, int id) { return get_size_of(h, id); }
int scl_iris_get_index(const scl_iris *h, int key, int8_t *robot, int *index) { return get_index(h, key, robot, index); }
int scl_iris_local_to_global(const scl_iris *h, int robot, int local, int *key) { return local_to_global(h, robot, local, key); }

int scl_iris_detect_intra(scl_iris *h, int cur, int *loop_id, float *bias, float *dist)
{
    if (!h || !loop_id || !bias) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    *loop_id = -1; *bias = 0.0f;
    if (dist) *dist = 10000000.0f;
    const std::vector<int> &mine = h->reg.keys_of(h->cfg.this_id);
    if (cur < 0 || cur >= (int)mine.size()) return fail(h, SCL_ERR_OUT_OF_RANGE, "detect_intra: no such keyframe of this robot");
    if (cur < h->cfg.num_exclude_recent + h->cfg.num_candidates + 1) return SCL_OK;     // D.h:1092-1095
    const int history = cur - h->cfg.num_exclude_recent;                                 // D.h:1097-1101
    std::vector<int> list(mine.begin(), mine.begin() + history);
    int pos, b; float d;
    int rc = detect_core_locked(h, mine[(size_t)cur], list, &pos, &d, &b);
    if (rc) return rc;
    if (dist) *dist = d;
    if ((double)d < h->cfg.dist_thres) { *loop_id = pos; *bias = (float)b; }             // D.h:1140-1144: the LOCAL index
    return SCL_OK;
}

int scl_iris_detect_inter(scl_iris *h, int cur, int *loop_id, float *bias, float *dist)
{
    if (!h || !loop_id || !bias) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    *loop_id = -1; *bias = 0.0f;
    if (dist) *dist = 10000000.0f;
    if (cur < 0 || cur >= h->reg.n) return fail(h, SCL_ERR_OUT_OF_RANGE, "detect_inter: key out of range");
    const std::vector<int> list = h->reg.inter_candidates(cur, h->cfg.this_id);        // newLocal2Global, D.h:1156-1195
    if ((int)list.size() < h->cfg.num_candidates + 1) return SCL_OK;                     // D.h:1198-1201
    int pos, b; float d;
    int rc = detect_core_locked(h, cur, list, &pos, &d, &b);
    if (rc) return rc;
    if (dist) *dist = d;
    if ((double)d < h->cfg.dist_thres && pos >= 0) { *loop_id = list[(size_t)pos]; *bias = (float)b; }   // D.h:1236, 1245-1248: the GLOBAL key
    return SCL_OK;
}

// ---- the batch forms (scl_iris.h): the handle's mutex for the whole call, everything on its stream
int scl_iris_make_and_save_many(scl_iris *h, const void *const *clouds, const int *n_points, int stride_bytes, const int8_t *robots, const int *indexs,
                                int count, float *out_values)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    return make_and_save_many_locked(h, clouds, n_points, stride_bytes, robots, indexs, count, out_values);
}

int scl_iris_save_from_wire_many(scl_iris *h, const float *values, const int8_t *robots, const int *indexs, int count)
{
    if (!h) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    return save_from_wire_many_locked(h, values, robots, indexs, count);
}

int scl_iris_detect_intra_many(scl_iris *h, const int *curs, int count, int *loop_ids, float *biases, float *dists)
{
    if (!h || count < 0 || (count > 0 && (!curs || !loop_ids || !biases))) return SCL_ERR_INVALID_ARG;
    if (count == 0) return SCL_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    return detect_intra_many_locked(h, curs, count, loop_ids, biases, dists);
}

int scl_iris_detect_inter_many(scl_iris *h, const int *curs, int count, int *loop_ids, float *biases, float *dists)
{
    if (!h || count < 0 || (count > 0 && (!curs || !loop_ids || !biases))) return SCL_ERR_INVALID_ARG;
    if (count == 0) return SCL_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    return detect_inter_many_locked(h, curs, count, loop_ids, biases, dists);
}

int scl_iris_make_save_and_detect(scl_iris *h, const void *const *clouds, const int *n_points, int stride_bytes, const int8_t *robots, const int *indexs,
                                  int count, int *loop_ids, float *biases, float *dists, float *out_values)
{
    if (!h || count < 0 || (count > 0 && (!loop_ids || !biases))) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    const int first = (int)h->reg.keys_of(h->cfg.this_id).size();
    int rc = make_and_save_many_locked(h, clouds, n_points, stride_bytes, robots, indexs, count, out_values);
    if (rc) return rc;
    std::vector<int> curs, at;                                                // the new keyframes of this robot: LOCAL index, entry of the call
    for (int i = 0; i < count; ++i)
        if (robots[i] == h->cfg.this_id) { curs.push_back(first + (int)curs.size()); at.push_back(i); }
    std::vector<int> loops(curs.size());
    std::vector<float> bs(curs.size()), ds(curs.size());
    if (!curs.empty() && (rc = detect_intra_many_locked(h, curs.data(), (int)curs.size(), loops.data(), bs.data(), ds.data()))) return rc;
    for (int i = 0; i < count; ++i) { loop_ids[i] = -1; biases[i] = 0.0f; if (dists) dists[i] = 10000000.0f; }
    for (size_t j = 0; j < at.size(); ++j) { loop_ids[at[j]] = loops[j]; biases[at[j]] = bs[j]; if (dists) dists[at[j]] = ds[j]; }
    return SCL_OK;
}

// ---- the exhaustive ranked search (scl_iris.h "THE EXHAUSTIVE SEARCH")
int scl_iris_search_intra(scl_iris *h, const int *curs, int count, int k, int *cand_ids, float *cand_biases, float *cand_dists, int *n_found)
{
    if (!h || count < 0 || (count > 0 && (!curs || !cand_ids))) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    return search_intra_locked(h, curs, count, k, cand_ids, cand_biases, cand_dists, n_found);
}

int scl_iris_search_inter(scl_iris *h, const int *curs, int count, int k, int *cand_ids, float *cand_biases, float *cand_dists, int *n_found)
{
    if (!h || count < 0 || (count > 0 && (!curs || !cand_ids))) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    return search_inter_locked(h, curs, count, k, cand_ids, cand_biases, cand_dists, n_found);
}

int scl_iris_get_image(scl_iris *h, int key, uint8_t *image, float *rowkey)
{
    if (!h || !image || !rowkey) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    if (key < 0 || key >= h->reg.n) return fail(h, SCL_ERR_OUT_OF_RANGE, "key out of range");
    const size_t cells = (size_t)h->cfg.rows * h->cfg.cols;
    SCL_HIP(h, hipMemcpyAsync(image, h->d_images + cells * key, cells, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipMemcpyAsync(rowkey, h->d_rowkeys + (size_t)h->cfg.rows * key, sizeof(float) * h->cfg.rows, hipMemcpyDeviceToHost, h->stream));
    SCL_HIP(h, hipStreamSynchronize(h->stream));
    return SCL_OK;
}

int scl_iris_get_feature(scl_iris *h, int key, uint8_t *T, uint8_t *M)
{
    if (!h || !T || !M) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    if (key < 0 || key >= h->reg.n) return fail(h, SCL_ERR_OUT_OF_RANGE, "key out of range");
    const size_t fw = (size_t)h->cfg.cols * h->words, tot = (size_t)h->trows * h->cfg.cols;
    for (int which = 0; which < 2; ++which) {
        hipLaunchKernelGGL(iris_unpack_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream,
                           (which ? h->d_M : h->d_T) + fw * key, h->cfg.cols, h->words, h->trows, h->d_unpack);
        SCL_HIP(h, hipGetLastError());
        SCL_HIP(h, hipMemcpyAsync(which ? M : T, h->d_unpack, tot, hipMemcpyDeviceToHost, h->stream));
        SCL_HIP(h, hipStreamSynchronize(h->stream));
    }
    return SCL_OK;
}

int scl_iris_hamming_batch(scl_iris *h, int key1, const int *cand, const int *scales, int n, float *dis, int *bias)
{
    if (!h || n < 0 || (n > 0 && (!cand || !scales || !dis || !bias))) return SCL_ERR_INVALID_ARG;
    if (n == 0) return SCL_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    std::vector<int> shifts((size_t)n * 5);
    for (int c = 0; c < n; ++c) for (int j = 0; j < 5; ++j) shifts[(size_t)c * 5 + j] = scales[c] - 2 + j;     // D.h:936
    return hamming_jobs_locked(h, key1, cand, shifts.data(), n, 5, dis, bias, true);
}

int scl_iris_hamming(scl_iris *h, int key1, int key2, int scale, float *dis, int *bias)
{
    return scl_iris_hamming_batch(h, key1, &key2, &scale, 1, dis, bias);
}

int scl_iris_fft_match(scl_iris *h, int key0, int roll0, int key1, float *center_x, int *compatible)
{
    if (!h || !center_x) return SCL_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    if (key0 < 0 || key0 >= h->reg.n || key1 < 0 || key1 >= h->reg.n) return fail(h, SCL_ERR_OUT_OF_RANGE, "fft_match: key out of range");
    const FftJob jb{key0, roll0, key1};
    return fft_match_jobs_locked(h, &jb, 1, center_x, compatible);
}

int scl_iris_compare(scl_iris *h, int key1, const int *cand, int n, float *dis, int *bias)
{
    if (!h || (n > 0 && (!cand || !dis || !bias)) || n < 0) return SCL_ERR_INVALID_ARG;
    if (n == 0) return SCL_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    if (key1 < 0 || key1 >= h->reg.n) return fail(h, SCL_ERR_OUT_OF_RANGE, "compare: key1 out of range");
    for (int i = 0; i < n; ++i) if (cand[i] < 0 || cand[i] >= h->reg.n) return fail(h, SCL_ERR_OUT_OF_RANGE, "compare: candidate out of range");
    return compare_jobs_locked(h, key1, cand, n, dis, bias);
}

int scl_iris_hamming_all_shifts(scl_iris *h, int key1, const int *cand, int n, float *dis, int *bias)
{
    if (!h || n < 0 || (n > 0 && (!cand || !dis || !bias))) return SCL_ERR_INVALID_ARG;
    if (n == 0) return SCL_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    const int N = h->cfg.cols;
    std::vector<int> shifts((size_t)n * N);
    for (int c = 0; c < n; ++c) for (int j = 0; j < N; ++j) shifts[(size_t)c * N + j] = j;
    return hamming_jobs_locked(h, key1, cand, shifts.data(), n, N, dis, bias, false);
}

}  // extern "C"
