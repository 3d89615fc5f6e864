/*
 * grsd_checker.c -- TEST INFRASTRUCTURE: the CPU restatement of the GRSD plugin (include/scl_grsd.h, DESIGN.md section 4 "GRSD"),
 * the yardstick of tests/test_gpu_grsd.py.  Built by the top-level Makefile with -O2 -ffp-contract=off and no -march, so every
 * float / double operation below is one correctly rounded IEEE operation in the order written.  Brute force throughout: every
 * stage of the contract is independent of traversal order, so no search structure is needed to state it.
 *
 *   grc_normals       radius neighbours by float d2 = (dx*dx + dy*dy) + dz*dz < (float)(r*r), the scatter as exact int64 sums of
 *                     rint(d * 2^20), fp64 covariance Sab - Sa*Sb/n, the device's cyclic Jacobi, PCL's float viewpoint flip;
 *   grc_voxels        pcl::VoxelGrid (oracle/icp_oracle.c's icpo_voxel_grid restated with the voxel indices kept);
 *   grc_rsd           per voxel centroid: nearest neighbour's normal as reference, acosf (tests/cpp/libfpfh_checker.so's fpc_acosf,
 *                     glibc's restated), min / max angle per distance bin, the radii and PCL's getSimpleType;
 *   grc_transitions   the 6 x 6 counters over the 26 neighbour cells of every centroid's cell;
 *   grc_histogram     the 21 floats;
 *   grc_describe      the chain.
 */
#include <float.h>
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

float fpc_acosf(float x);   /* tests/cpp/libfpfh_checker.so */

static inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline const float *pt(const void *pts, int stride, int i) { return (const float *)((const char *)pts + (size_t)i * (size_t)stride); }

static inline float d2f(const float *a, const float *b)
{
    const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    return (dx * dx + dy * dy) + dz * dz;
}

/* the device's jacobi3 (csrc/device_common.hpp) */
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

/* ---- normals ------------------------------------------------------------------------------------------------------------------ */
/* the normal of point q over ALL points within the radius (q included): out[3], returns validity */
static int normal_one(const void *pts, int n, int stride, int q, float r2, float *out)
{
    const float *a = pt(pts, stride, q);
    int64_t cnt = 0, s[3] = {0, 0, 0}, s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0;
    for (int j = 0; j < n; j++) {
        const float *b = pt(pts, stride, j);
        const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (!(d2 < r2)) continue;
        const int64_t qa = (int64_t)rint((double)dx * 1048576.0), qb = (int64_t)rint((double)dy * 1048576.0),
                      qc = (int64_t)rint((double)dz * 1048576.0);
        cnt++; s[0] += qa; s[1] += qb; s[2] += qc;
        s00 += qa * qa; s01 += qa * qb; s02 += qa * qc; s11 += qb * qb; s12 += qb * qc; s22 += qc * qc;
    }
    if (cnt < 3) { out[0] = out[1] = out[2] = u2f(0x7fc00000u); return 0; }
    const double dn = (double)cnt, m0 = (double)s[0], m1 = (double)s[1], m2 = (double)s[2];
    const double c00 = (double)s00 - m0 * m0 / dn, c01 = (double)s01 - m0 * m1 / dn, c02 = (double)s02 - m0 * m2 / dn,
                 c11 = (double)s11 - m1 * m1 / dn, c12 = (double)s12 - m1 * m2 / dn, c22 = (double)s22 - m2 * m2 / dn;
    double m[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}}, v[3][3];
    jacobi3(m, v);
    int k = 0;
    if (m[1][1] < m[k][k]) k = 1;
    if (m[2][2] < m[k][k]) k = 2;
    float nx = (float)v[0][k], ny = (float)v[1][k], nz = (float)v[2][k];
    const float vx = 0.0f - a[0], vy = 0.0f - a[1], vz = 0.0f - a[2];
    if ((vx * nx + vy * ny) + vz * nz < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    out[0] = nx; out[1] = ny; out[2] = nz;
    return 1;
}

typedef struct {
    const void *pts; int n, stride; const int *queries; int q0, q1; float r2; float *normals; uint8_t *valid;
} normal_job;

static void *normal_run(void *arg)
{
    normal_job *j = (normal_job *)arg;
    for (int t = j->q0; t < j->q1; t++)
        j->valid[t] = (uint8_t)normal_one(j->pts, j->n, j->stride, j->queries ? j->queries[t] : t, j->r2, j->normals + (size_t)3 * t);
    return NULL;
}

/* normals of the queries (NULL: all n points), nq x 3 floats and nq validity flags */
int grc_normals(const void *pts, int n, int stride, double ne_radius, const int *queries, int nq, int nthreads, float *normals, uint8_t *valid)
{
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    pthread_t th[64];
    normal_job jobs[64];
    for (int t = 0; t < nthreads; t++) {
        normal_job jb = {pts, n, stride, queries, (int)((long long)nq * t / nthreads), (int)((long long)nq * (t + 1) / nthreads),
                         (float)(ne_radius * ne_radius), normals, valid};
        jobs[t] = jb;
        if (pthread_create(&th[t], NULL, normal_run, &jobs[t])) return -1;
    }
    for (int t = 0; t < nthreads; t++) pthread_join(th[t], NULL);
    return 0;
}

/* ---- voxels ------------------------------------------------------------------------------------------------------------------- */
typedef struct { long long idx; int pt; } vox_key;
static int cmp_vox(const void *a, const void *b)
{
    const vox_key *x = (const vox_key *)a, *y = (const vox_key *)b;
    if (x->idx != y->idx) return x->idx < y->idx ? -1 : 1;
    return (x->pt > y->pt) - (x->pt < y->pt);
}

/* centroids (room for n x 3 floats) and voxel indices (room for n) in ascending voxel index; grid[6] = min_b, div_b.  Returns the
 * number of voxels, -1 when the voxel index range overflows int32, -2 for a non-finite coordinate */
int grc_voxels(const void *pts, int n, int stride, float leaf, float *cent, int32_t *vidx, int32_t *grid)
{
    const float inv = 1.0f / leaf;
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = 0; i < n; i++) {
        const float *p = pt(pts, stride, i);
        if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) return -2;
        for (int a = 0; a < 3; a++) { if (p[a] < mn[a]) mn[a] = p[a]; if (p[a] > mx[a]) mx[a] = p[a]; }
    }
    long long minb[3], divb[3];
    for (int a = 0; a < 3; a++) {
        const float lo = floorf(mn[a] * inv), hi = floorf(mx[a] * inv);
        if (!(lo >= -2147483648.f && hi <= 2147483520.f)) return -1;
        minb[a] = (long long)lo;
        divb[a] = (long long)hi - minb[a] + 1;
        if (divb[a] > 2147483647LL) return -1;
    }
    if (divb[0] * divb[1] > 2147483647LL || divb[0] * divb[1] * divb[2] > 2147483647LL) return -1;
    vox_key *keys = (vox_key *)malloc(sizeof(vox_key) * (size_t)n);
    if (!keys) return -3;
    for (int i = 0; i < n; i++) {
        const float *p = pt(pts, stride, i);
        const long long i0 = (long long)floorf(p[0] * inv) - minb[0], i1 = (long long)floorf(p[1] * inv) - minb[1],
                        i2 = (long long)floorf(p[2] * inv) - minb[2];
        keys[i].idx = i0 + i1 * divb[0] + i2 * divb[0] * divb[1];
        keys[i].pt = i;
    }
    qsort(keys, (size_t)n, sizeof(vox_key), cmp_vox);
    int nout = 0;
    for (int a = 0; a < n; ) {
        int b = a;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        while (b < n && keys[b].idx == keys[a].idx) {
            const float *p = pt(pts, stride, keys[b].pt);
            sx += p[0]; sy += p[1]; sz += p[2];
            b++;
        }
        const float cnt = (float)(b - a);
        cent[3 * nout] = sx / cnt; cent[3 * nout + 1] = sy / cnt; cent[3 * nout + 2] = sz / cnt;
        vidx[nout] = (int32_t)keys[a].idx;
        nout++;
        a = b;
    }
    free(keys);
    for (int a = 0; a < 3; a++) { grid[a] = (int32_t)minb[a]; grid[3 + a] = (int32_t)divb[a]; }
    return nout;
}

/* ---- RSD ---------------------------------------------------------------------------------------------------------------------- */
/* PCL's getSimpleType on the float radii (thresholds as doubles): 0 noise, 1 plane, 2 cylinder, 3 sphere, 4 edge */
int grc_simple_type(float r_min, float r_max)
{
    if ((double)r_min > 0.1) return 1;
    if ((double)r_max > 0.175) return 2;
    if ((double)r_min < 0.015) return 0;
    if ((double)(r_max - r_min) < 0.05) return 3;
    return 4;
}

static void rsd_one(const void *pts, int n, int stride, const float *normals, const uint8_t *valid, const float *c, double max_dist,
                    float *r_min, float *r_max)
{
    const float r2 = (float)(max_dist * max_dist);
    const float pi = u2f(0x40490fdbu), pio2 = u2f(0x3fc90fdbu);
    uint64_t best = ~0ull;
    int count = 0;
    for (int j = 0; j < n; j++) {
        const float d2 = d2f(c, pt(pts, stride, j));
        if (!(d2 < r2)) continue;
        count++;
        const uint64_t key = ((uint64_t)f2u(d2) << 32) | (uint32_t)j;
        if (key < best) best = key;
    }
    *r_min = *r_max = 0.0f;
    if (count < 2) return;
    uint32_t mn[5] = {0u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[5] = {0u, 0u, 0u, 0u, 0u};
    const int ref = (int)(uint32_t)best;
    if (valid[ref]) {
        const float *a = normals + (size_t)3 * ref;
        for (int j = 0; j < n; j++) {
            const float d2 = d2f(c, pt(pts, stride, j));
            if (!(d2 < r2) || !valid[j]) continue;
            const float *b = normals + (size_t)3 * j;
            float cosine = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
            cosine = cosine > 1.0f ? 1.0f : (cosine < -1.0f ? -1.0f : cosine);
            float angle = fpc_acosf(cosine);
            if (angle > pio2) angle = pi - angle;
            const double dist = sqrt((double)d2);
            int bin = (int)floor(5.0 * dist / max_dist);
            if (bin > 4) bin = 4;
            const uint32_t ab = f2u(angle);
            if (ab < mn[bin]) mn[bin] = ab;
            if (ab > mx[bin]) mx[bin] = ab;
        }
    }
    double amin = 0.0, amin_d = 0.0, amax = 0.0, amax_d = 0.0;
    for (int k = 0; k < 5; k++) {
        if (mn[k] == 0xffffffffu) continue;
        const double f = ((double)k + 0.5) * max_dist / 5.0;
        const double pmin = (double)u2f(mn[k]), pmax = (double)u2f(mx[k]);
        amin += pmin * pmin; amin_d += pmin * f;
        amax += pmax * pmax; amax_d += pmax * f;
    }
    const double plane_radius = 0.2;
    const double ra = amin == 0.0 ? plane_radius : fmin(amin_d / amin, plane_radius);
    const double rb = amax == 0.0 ? plane_radius : fmin(amax_d / amax, plane_radius);
    float fa = (float)ra, fb = (float)rb;
    fa = (float)((double)fa * 1.1); fb = (float)((double)fb * 1.1);
    *r_min = fa < fb ? fa : fb; *r_max = fa < fb ? fb : fa;
}

typedef struct {
    const void *pts; int n, stride; const float *normals; const uint8_t *valid; const float *cent; const int *queries; int q0, q1;
    double max_dist; float *r_min, *r_max; int32_t *cls;
} rsd_job;

static void *rsd_run(void *arg)
{
    rsd_job *j = (rsd_job *)arg;
    for (int t = j->q0; t < j->q1; t++) {
        const int v = j->queries ? j->queries[t] : t;
        rsd_one(j->pts, j->n, j->stride, j->normals, j->valid, j->cent + (size_t)3 * v, j->max_dist, &j->r_min[t], &j->r_max[t]);
        j->cls[t] = grc_simple_type(j->r_min[t], j->r_max[t]);
    }
    return NULL;
}

/* r_min, r_max and the class of the voxels `queries` (NULL: all nvox) from the normals (n x 3, validity n) and the centroids */
int grc_rsd(const void *pts, int n, int stride, const float *normals, const uint8_t *valid, const float *cent, double grsd_radius,
            const int *queries, int nq, int nthreads, float *r_min, float *r_max, int32_t *cls)
{
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    pthread_t th[64];
    rsd_job jobs[64];
    for (int t = 0; t < nthreads; t++) {
        rsd_job jb = {pts, n, stride, normals, valid, cent, queries, (int)((long long)nq * t / nthreads),
                      (int)((long long)nq * (t + 1) / nthreads), grsd_radius, r_min, r_max, cls};
        jobs[t] = jb;
        if (pthread_create(&th[t], NULL, rsd_run, &jobs[t])) return -1;
    }
    for (int t = 0; t < nthreads; t++) pthread_join(th[t], NULL);
    return 0;
}

/* ---- transitions and the histogram -------------------------------------------------------------------------------------------- */
/* T[36]: for every voxel and each of the 26 cells around the cell OF ITS CENTROID: T[class][neighbour's class, 5 when the cell is
 * outside the grid or unoccupied]++.  vidx: the occupied voxel indices, ascending */
void grc_transitions(const float *cent, const int32_t *vidx, const int32_t *cls, int nvox, float leaf, const int32_t *grid, uint32_t *T)
{
    const float inv = 1.0f / leaf;
    memset(T, 0, sizeof(uint32_t) * 36);
    for (int v = 0; v < nvox; v++) {
        long long cc[3];
        for (int a = 0; a < 3; a++) cc[a] = (long long)floorf(cent[3 * v + a] * inv) - grid[a];
        for (int o = 0; o < 27; o++) {
            if (o == 13) continue;
            const long long x = cc[0] + (o % 3 - 1), y = cc[1] + (o / 3 % 3 - 1), z = cc[2] + (o / 9 - 1);
            int other = 5;
            if (x >= 0 && x < grid[3] && y >= 0 && y < grid[4] && z >= 0 && z < grid[5]) {
                const long long key = x + y * grid[3] + z * (long long)grid[3] * grid[4];
                int a = 0, b = nvox;
                while (a < b) { const int m = (a + b) >> 1; if (vidx[m] < key) a = m + 1; else b = m; }
                if (a < nvox && vidx[a] == key) other = cls[a];
            }
            T[cls[v] * 6 + other]++;
        }
    }
}

void grc_histogram(const uint32_t *T, float *out)
{
    int k = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) out[k++] = (float)(uint32_t)(T[i * 6 + j] + T[j * 6 + i]);
}

/* the whole descriptor of one cloud -> out[21], T[36] (may be NULL); 0, or grc_voxels' negative status */
int grc_describe(const void *pts, int n, int stride, double ne_radius, double grsd_radius, int nthreads, float *out, uint32_t *T_out)
{
    if (n < 1) return -4;
    float *cent = (float *)malloc(sizeof(float) * 3 * (size_t)n), *normals = (float *)malloc(sizeof(float) * 3 * (size_t)n);
    float *rr = (float *)malloc(sizeof(float) * 2 * (size_t)n);
    int32_t *vidx = (int32_t *)malloc(sizeof(int32_t) * 2 * (size_t)n), grid[6];
    uint8_t *valid = (uint8_t *)malloc((size_t)n);
    int rc = -3;
    if (cent && normals && rr && vidx && valid) {
        const int nvox = grc_voxels(pts, n, stride, (float)grsd_radius, cent, vidx, grid);
        rc = nvox < 0 ? nvox : 0;
        if (rc == 0) rc = grc_normals(pts, n, stride, ne_radius, NULL, n, nthreads, normals, valid);
        if (rc == 0) rc = grc_rsd(pts, n, stride, normals, valid, cent, grsd_radius, NULL, nvox, nthreads, rr, rr + n, vidx + n);
        if (rc == 0) {
            uint32_t T[36];
            grc_transitions(cent, vidx, vidx + n, nvox, (float)grsd_radius, grid, T);
            grc_histogram(T, out);
            if (T_out) memcpy(T_out, T, sizeof T);
        }
    }
    free(cent); free(normals); free(rr); free(vidx); free(valid);
    return rc;
}
