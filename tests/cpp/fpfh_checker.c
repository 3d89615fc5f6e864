/*
 * fpfh_checker.c -- TEST INFRASTRUCTURE: the CPU restatement of the FPFH plugin (include/scl_fpfh.h, DESIGN.md section 4 "FPFH"),
 * the yardstick of tests/test_gpu_fpfh.py.  Built by the top-level Makefile with -O2 -ffp-contract=off and no -march, so every
 * float / double operation below is one correctly rounded IEEE operation in the order written.
 *
 *   fpc_acosf            glibc 2.35's float acosf (sysdeps/ieee754/flt-32/e_acosf.c, fdlibm's algorithm) restated one operation at
 *                        a time; fpc_acosf_exhaustive compares it with libm on all 2^32 inputs and forms the block checksums of
 *                        tests/golden/acosf_blocks.json (the device's copy is checked against those);
 *   fpc_knn              brute-force k nearest by (float d2 = (dx*dx + dy*dy) + dz*dz, index);
 *   fpc_normals          fp64 mean and scatter in (d2, index) order, the cyclic Jacobi of the device, the smallest eigenvalue's
 *                        column rounded to float, flipped towards the origin by PCL's float test;
 *   fpc_pair_features    PCL's computePairFeatures in Eigen's Vector4f operation order; atan2f = oracle/liboracle.so's
 *                        iriso_atan2f (glibc's atan2f restated);
 *   fpc_spfh_counts      the SPFH of the last point over the pairs [0, N - 2]: 3 x 11 integer bin counts and the skipped pairs;
 *   fpc_hist_value_loop  the float left after `count` sequential `+= hist_incr` (what PCL's histogram holds).
 */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

float iriso_atan2f(float y, float x);   /* oracle/liboracle.so */

static inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

/* ---- acosf ------------------------------------------------------------------------------------------------------------------ */
float fpc_acosf(float x)
{
    const float one = 1.0f, pi = u2f(0x40490fda), pio2_hi = u2f(0x3fc90fda), pio2_lo = u2f(0x33a22168);
    const float pS0 = u2f(0x3e2aaaab), pS1 = u2f(0xbea6b090), pS2 = u2f(0x3e4e0aa8), pS3 = u2f(0xbd241146), pS4 = u2f(0x3a4f7f04),
                pS5 = u2f(0x3811ef08);
    const float qS1 = u2f(0xc019d139), qS2 = u2f(0x4001572d), qS3 = u2f(0xbf303361), qS4 = u2f(0x3d9dc62e);
    const int32_t hx = (int32_t)f2u(x), ix = hx & 0x7fffffff;
    float z, p, q, r, w, s, c, df;
    if (ix == 0x3f800000) return hx > 0 ? 0.0f : pi + 2.0f * pio2_lo;    /* |x| = 1 */
    if (ix > 0x3f800000) return (x - x) / (x - x);                       /* |x| > 1 or NaN */
    if (ix < 0x3f000000) {                                                /* |x| < 0.5 */
        if (ix <= 0x32800000) return pio2_hi + pio2_lo;                   /* |x| <= 2^-26 */
        z = x * x;
        p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        r = p / q;
        return pio2_hi - (x - (pio2_lo - x * r));
    }
    if (hx < 0) {                                                         /* x < -0.5 */
        z = (one + x) * 0.5f;
        p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        s = sqrtf(z);
        r = p / q;
        w = r * s - pio2_lo;
        return pi - 2.0f * (s + w);
    }
    z = (one - x) * 0.5f;                                                 /* x > 0.5 */
    s = sqrtf(z);
    df = u2f(f2u(s) & 0xfffff000u);
    c = (z - df * df) / (s + df);
    p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    r = p / q;
    w = r * s + c;
    return 2.0f * (df + w);
}

/* block checksum, as tests/golden/atanf_blocks.json: sum mod 2^64 of splitmix64((bits << 32) | result bits), NaN as 0x7fc00000 */
static inline uint64_t mix64(uint64_t z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

typedef struct { int b0, b1; uint64_t *blocks; uint64_t diffs; } acos_job;

static void *acos_run(void *arg)
{
    acos_job *j = (acos_job *)arg;
    for (int b = j->b0; b < j->b1; b++) {
        uint64_t h = 0;
        for (uint32_t i = 0; i < (1u << 24); i++) {
            const uint32_t bits = ((uint32_t)b << 24) | i;
            const float x = u2f(bits), a = fpc_acosf(x), l = acosf(x);
            uint32_t ua = f2u(a), ul = f2u(l);
            if (a != a) ua = 0x7fc00000u;
            if (l != l) ul = 0x7fc00000u;
            j->diffs += ua != ul;
            h += mix64(((uint64_t)bits << 32) | ua);
        }
        j->blocks[b] = h;
    }
    return NULL;
}

/* all 2^32 inputs: the number of results that differ from libm's acosf, and the 256 block checksums of fpc_acosf */
int fpc_acosf_exhaustive(int nthreads, uint64_t *blocks, uint64_t *diffs)
{
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    pthread_t th[64];
    acos_job jobs[64];
    for (int t = 0; t < nthreads; t++) {
        jobs[t].b0 = 256 * t / nthreads; jobs[t].b1 = 256 * (t + 1) / nthreads; jobs[t].blocks = blocks; jobs[t].diffs = 0;
        if (pthread_create(&th[t], NULL, acos_run, &jobs[t])) return -1;
    }
    *diffs = 0;
    for (int t = 0; t < nthreads; t++) { pthread_join(th[t], NULL); *diffs += jobs[t].diffs; }
    return 0;
}

/* ---- neighbours and normals ---------------------------------------------------------------------------------------------- */
static inline const float *pt(const void *pts, int stride, int i) { return (const float *)((const char *)pts + (size_t)i * (size_t)stride); }

static inline float d2f(const float *a, const float *b)
{
    const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    return (dx * dx + dy * dy) + dz * dz;
}

/* the k = min(10, n) nearest of point q by (d2, index); idx / d2 hold k entries */
static void knn_one(const void *pts, int n, int stride, int q, int k, int *idx, float *d2)
{
    uint64_t best[10];
    for (int j = 0; j < 10; j++) best[j] = ~0ull;
    const float *a = pt(pts, stride, q);
    for (int i = 0; i < n; i++) {
        const uint64_t key = ((uint64_t)f2u(d2f(a, pt(pts, stride, i))) << 32) | (uint32_t)i;
        if (key >= best[k - 1]) continue;
        int j = k - 1;
        while (j > 0 && best[j - 1] > key) { best[j] = best[j - 1]; j--; }
        best[j] = key;
    }
    for (int j = 0; j < k; j++) { idx[j] = (int)(uint32_t)best[j]; d2[j] = u2f((uint32_t)(best[j] >> 32)); }
}

/* queries (NULL: all n points, in order), nq of them: idx / d2 are nq x min(10, n) */
void fpc_knn(const void *pts, int n, int stride, const int *queries, int nq, int *idx, float *d2)
{
    const int k = n < 10 ? n : 10;
    for (int t = 0; t < nq; t++) knn_one(pts, n, stride, queries ? queries[t] : t, k, idx + (size_t)t * k, d2 + (size_t)t * k);
}

static void jacobi3(double a[3][3], double v[3][3])
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
        const double diag = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]);
        if (off == 0.0 || off <= 1e-300 || off < 1e-18 * diag) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                double t;
                if (fabs(theta) > 1e150) t = 0.5 / theta;
                else t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq; v[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

/* the normal of point q from its neighbour list (k entries in (d2, index) order) */
void fpc_normal_from(const void *pts, int stride, int q, const int *nb, int k, float *out)
{
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int j = 0; j < k; j++) { const float *p = pt(pts, stride, nb[j]); sx += (double)p[0]; sy += (double)p[1]; sz += (double)p[2]; }
    const double mx = sx / (double)k, my = sy / (double)k, mz = sz / (double)k;
    double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
    for (int j = 0; j < k; j++) {
        const float *p = pt(pts, stride, nb[j]);
        const double dx = (double)p[0] - mx, dy = (double)p[1] - my, dz = (double)p[2] - mz;
        c00 += dx * dx; c01 += dx * dy; c02 += dx * dz; c11 += dy * dy; c12 += dy * dz; c22 += dz * dz;
    }
    double a[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}}, v[3][3];
    jacobi3(a, v);
    int m = 0;
    if (a[1][1] < a[m][m]) m = 1;
    if (a[2][2] < a[m][m]) m = 2;
    float nx = (float)v[0][m], ny = (float)v[1][m], nz = (float)v[2][m];
    const float *p = pt(pts, stride, q);
    const float vx = 0.0f - p[0], vy = 0.0f - p[1], vz = 0.0f - p[2];
    if ((vx * nx + vy * ny) + vz * nz < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    out[0] = nx; out[1] = ny; out[2] = nz;
}

/* normals of the queries (NULL: all n points), nq x 3 */
void fpc_normals(const void *pts, int n, int stride, const int *queries, int nq, float *normals)
{
    const int k = n < 10 ? n : 10;
    int idx[10]; float d2[10];
    for (int t = 0; t < nq; t++) {
        const int q = queries ? queries[t] : t;
        knn_one(pts, n, stride, q, k, idx, d2);
        fpc_normal_from(pts, stride, q, idx, k, normals + (size_t)3 * t);
    }
}

/* ---- pair features and the SPFH ------------------------------------------------------------------------------------------ */
/* Eigen's Vector4f dot with lane 3 = +0: (a0*b0 + a2*b2) + (a1*b1 + 0) */
static inline float dot4(const float *a, const float *b) { return (a[0] * b[0] + a[2] * b[2]) + (a[1] * b[1] + 0.0f); }
static inline void cross3(const float *a, const float *b, float *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

/* PCL's computePairFeatures(p1, n1, p2, n2): 1 and f[0..3] = (f1, f2, f3, f4), or 0 when the pair is skipped (f4 == 0 or
 * |dp x n1| == 0) */
int fpc_pair_features(const float *p1, const float *n1, const float *p2, const float *n2, float *f)
{
    float dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const float f4 = sqrtf(dot4(dp, dp));
    f[0] = f[1] = f[2] = f[3] = 0.0f;
    if (f4 == 0.0f) return 0;
    const float a1 = dot4(n1, dp) / f4, a2 = dot4(n2, dp) / f4;
    const float *u = n1, *m = n2;
    float f3;
    if (fpc_acosf(fabsf(a1)) > fpc_acosf(fabsf(a2))) {
        u = n2; m = n1;
        dp[0] = -dp[0]; dp[1] = -dp[1]; dp[2] = -dp[2];
        f3 = -a2;
    } else {
        f3 = a1;
    }
    float v[3], w[3];
    cross3(dp, u, v);
    const float vn = sqrtf(dot4(v, v));
    if (vn == 0.0f) return 0;
    v[0] = v[0] / vn; v[1] = v[1] / vn; v[2] = v[2] / vn;
    cross3(u, v, w);
    f[1] = dot4(v, m);
    f[0] = iriso_atan2f(dot4(w, m), dot4(u, m));
    f[2] = f3; f[3] = f4;
    return 1;
}

static inline int clamp_bin(double t)
{
    if (t != t) return 0;
    const double fl = floor(t);
    if (fl < 0.0) return 0;
    if (fl >= 11.0) return 10;
    return (int)fl;
}

/* the three bins of a pair: f1 by floor(11 * ((f1 + M_PI) * d_pi)), f2 / f3 by floor(11 * ((f + 1.0) * 0.5)), all in double */
void fpc_bins(const float *f, int *b)
{
    const float d_pi = 1.0f / (2.0f * (float)M_PI);
    b[0] = clamp_bin(11.0 * (((double)f[0] + M_PI) * (double)d_pi));
    b[1] = clamp_bin(11.0 * (((double)f[1] + 1.0) * 0.5));
    b[2] = clamp_bin(11.0 * (((double)f[2] + 1.0) * 0.5));
}

/* the SPFH of the last point against the points [0, n - 2]: counts[33] (f1 bins, f2 bins, f3 bins), *skipped pairs */
void fpc_spfh_counts(const void *pts, int n, int stride, const float *normals, uint32_t *counts, uint32_t *skipped)
{
    memset(counts, 0, sizeof(uint32_t) * 33);
    *skipped = 0;
    const float *pl = pt(pts, stride, n - 1), *nl = normals + (size_t)3 * (n - 1);
    for (int j = 0; j <= n - 2; j++) {
        float f[4];
        int b[3];
        if (!fpc_pair_features(pl, nl, pt(pts, stride, j), normals + (size_t)3 * j, f)) { (*skipped)++; continue; }
        fpc_bins(f, b);
        counts[b[0]]++; counts[11 + b[1]]++; counts[22 + b[2]]++;
    }
}

/* ---- histogram values ----------------------------------------------------------------------------------------------------- */
float fpc_hist_value_loop(uint32_t count, float inc)
{
    float s = 0.0f;
    for (uint32_t i = 0; i < count; i++) s += inc;
    return s;
}

/* out[c] = the value after c additions, c = 0 .. nmax */
void fpc_hist_values_prefix(int nmax, float inc, float *out)
{
    float s = 0.0f;
    out[0] = s;
    for (int c = 1; c <= nmax; c++) { s += inc; out[c] = s; }
}

/* the whole descriptor of one cloud: brute-force normals, SPFH counts, sequential values -> out[33] */
int fpc_describe(const void *pts, int n, int stride, float *out, uint32_t *counts_out, uint32_t *skipped_out)
{
    if (n < 3) return -1;
    float *normals = (float *)malloc(sizeof(float) * 3 * (size_t)n);
    if (!normals) return -2;
    fpc_normals(pts, n, stride, NULL, n, normals);
    uint32_t counts[33], skipped;
    fpc_spfh_counts(pts, n, stride, normals, counts, &skipped);
    free(normals);
    const float inc = 100.0f / (float)(long long)(n - 2);
    for (int b = 0; b < 33; b++) out[b] = fpc_hist_value_loop(counts[b], inc);
    if (counts_out) memcpy(counts_out, counts, sizeof counts);
    if (skipped_out) *skipped_out = skipped;
    return 0;
}
