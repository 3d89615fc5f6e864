// pcm.hip -- pairwise consistency maximisation over the loop closures of one pair of trajectories (contract: include/scl_engine.h
// "PAIRWISE CONSISTENCY OF LOOP CLOSURES"): the d^2 matrix of the N (N - 1) / 2 cycle tests in fp64, the consistency graph as N x W
// words, and the greedy maximum clique of the contract on those words.
//
//   pcm_prep_kernel        one thread per keyframe pose and per loop: quaternions normalised, Z_i^-1, Ad(Z_i) Sigma_i Ad(Z_i)^T
//   pcm_pairs_kernel       one thread per pair (i, j), j = 64 w + lane of the wave that owns word w of row i; the wave's ballot IS that word
//                          of the upper triangle (a plain store: every word of every row is written, the ones below the diagonal as 0)
//   pcm_symmetrise_kernel  one wave per row: the lower triangle's bits gathered from the upper words by ballot, the degree
//   pcm_clique_kernel      one wave per seed, P as one word per lane
//   pcm_clique_finish_kernel  the winner (largest, then lowest seed), its members in ascending order
//
// No floating-point atomics and no atomics on the graph at all; the one integer atomic is the size of the largest clique found so far,
// which lets a seed that could not even tie leave at once (the answer does not depend on when it is read: see the kernel).
#include "pcm.hpp"
#include "se3_device.hpp"

#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

namespace scl {

namespace {

using namespace se3;               // the quaternion, composition and adjoint helpers shared with pgo.hip; a pose is kPoseStride doubles

constexpr int kLoopStride = 56;    // q, t of Z (7); q, t of Z^-1 (7); Ad(Z) Sigma Ad(Z)^T upper triangle (21); Sigma upper triangle (21)
constexpr int kLoopZinv = 7, kLoopS = 14, kLoopRaw = 35;

// out = upper triangle of Ad(q, t) S Ad(q, t)^T for Ad = [[R, 0], [B, R]], B = [t]x R, and S = [[P, Q], [Q^T, U]] given by its upper
// triangle: TL = (R P) R^T, TR = (R P) B^T + (R Q) R^T, BR = (B P + R Q^T) B^T + (B Q + R U) R^T
__device__ inline void adjoint_cov(const double *q, const double *t, const double *S, double *out)
{
    double R[9], B[9], P[9], Q[9], U[9];
    adjoint_blocks(q, t, R, B);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            P[3 * r + c] = r <= c ? S[tri(r, c)] : S[tri(c, r)];
            Q[3 * r + c] = S[tri(r, 3 + c)];
            U[3 * r + c] = r <= c ? S[tri(3 + r, 3 + c)] : S[tri(3 + c, 3 + r)];
        }
    double RP[9], RQ[9], W1[9], W2[9], X[9], Y[9];
    mm(R, P, RP); mm(R, Q, RQ);
    mm(B, P, X); mmt(R, Q, Y);
#pragma unroll
    for (int k = 0; k < 9; ++k) W1[k] = X[k] + Y[k];
    mm(B, Q, X); mm(R, U, Y);
#pragma unroll
    for (int k = 0; k < 9; ++k) W2[k] = X[k] + Y[k];
    mmt(RP, R, X);                                                            // TL
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = r; c < 3; ++c) out[tri(r, c)] = X[3 * r + c];
    mmt(RP, B, X); mmt(RQ, R, Y);                                             // TR
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[tri(r, 3 + c)] = X[3 * r + c] + Y[3 * r + c];
    mmt(W1, B, X); mmt(W2, R, Y);                                             // BR
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = r; c < 3; ++c) out[tri(3 + r, 3 + c)] = X[3 * r + c] + Y[3 * r + c];
}

__global__ __launch_bounds__(256) void pcm_prep_kernel(const double *poses_a, int n_a, const double *poses_b, int n_b,
                                                        const double *z, const double *cov, int n,
                                                        double *prep_a, double *prep_b, double *loops)
{
    int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t < n_a) { double o[7]; normalise_pose(poses_a + 7 * (size_t)t, o); for (int k = 0; k < 7; ++k) prep_a[kPoseStride * (size_t)t + k] = o[k]; return; }
    t -= n_a;
    if (t < n_b) { double o[7]; normalise_pose(poses_b + 7 * (size_t)t, o); for (int k = 0; k < 7; ++k) prep_b[kPoseStride * (size_t)t + k] = o[k]; return; }
    t -= n_b;
    if (t >= n) return;
    double Z[7], qi[4], ti[3], S[21], A[21];
    normalise_pose(z + 7 * (size_t)t, Z);
    qconj(Z, qi);
    qrot(qi, Z + 4, ti);
    const double *c = cov + 36 * (size_t)t;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) S[tri(a, b)] = c[6 * a + b];
    adjoint_cov(Z, Z + 4, S, A);
    double *o = loops + kLoopStride * (size_t)t;
    for (int k = 0; k < 7; ++k) o[k] = Z[k];
    for (int k = 0; k < 4; ++k) o[kLoopZinv + k] = qi[k];
    for (int k = 0; k < 3; ++k) o[kLoopZinv + 4 + k] = -ti[k];
    for (int k = 0; k < 21; ++k) { o[kLoopS + k] = A[k]; o[kLoopRaw + k] = S[k]; }
}

__device__ double pair_d2(const double *prep_a, const double *prep_b, const int *idx_a, const int *idx_b, const double *loops,
                          const double *odom, int i, int j)
{
    const int ai = idx_a[i], aj = idx_a[j], bi = idx_b[i], bj = idx_b[j];
    const double *Li = loops + kLoopStride * (size_t)i, *Lj = loops + kLoopStride * (size_t)j;
    const double *Xai = prep_a + kPoseStride * (size_t)ai, *Xaj = prep_a + kPoseStride * (size_t)aj;
    const double *Xbi = prep_b + kPoseStride * (size_t)bi, *Xbj = prep_b + kPoseStride * (size_t)bj;
    double qA[4], tA[3], qB[4], tB[3], qBi[4], tBi[3];
    relative_pose(Xai, Xaj, qA, tA);                       // T_A    = (X^A_ai)^-1 X^A_aj
    relative_pose(Xbj, Xbi, qB, tB);                       // T_B    = (X^B_bj)^-1 X^B_bi
    relative_pose(Xbi, Xbj, qBi, tBi);                     // T_B^-1
    double q1[4], t1[3], q2[4], t2[3], qE[4], tE[3], qM[4], tM[3];
    compose(qA, tA, Lj, Lj + 4, q1, t1);                   // T_A Z_j
    compose(q1, t1, qB, tB, q2, t2);                       // T_A Z_j T_B
    compose(q2, t2, Li + kLoopZinv, Li + kLoopZinv + 4, qE, tE);   // E
    compose(Li, Li + 4, qBi, tBi, qM, tM);                 // M = Z_i T_B^-1
    // r = (Log_SO3, t)
    double r[6];
    {
        double qp[4], nv;
        qlog(qE, r, qp, &nv);
        r[3] = tE[0]; r[4] = tE[1]; r[5] = tE[2];
    }
    // Sigma
    double Sj[21], S[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) Sj[k] = Lj[kLoopRaw + k];
    adjoint_cov(qM, tM, Sj, S);
    const double steps = fabs((double)ai - (double)aj) + fabs((double)bi - (double)bj);
#pragma unroll
    for (int k = 0; k < 21; ++k) S[k] = Li[kLoopS + k] + S[k];
#pragma unroll
    for (int a = 0; a < 6; ++a) S[tri(a, a)] = S[tri(a, a)] + odom[a] * steps;
    // Cholesky S = L L^T, L y = r, d2 = y . y
    double L[21], y[6];                                    // L[tri(c, r)] = L_rc, r >= c
    double d2 = 0.0;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double s = S[tri(c, c)];
#pragma unroll
        for (int k = 0; k < c; ++k) s -= L[tri(k, c)] * L[tri(k, c)];
        if (!(s > 0.0)) ok = false;
        const double p = sqrt(s);
        L[tri(c, c)] = p;
#pragma unroll
        for (int rr = c + 1; rr < 6; ++rr) {
            double v = S[tri(c, rr)];
#pragma unroll
            for (int k = 0; k < c; ++k) v -= L[tri(k, rr)] * L[tri(k, c)];
            L[tri(c, rr)] = v / p;
        }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double v = r[a];
#pragma unroll
        for (int k = 0; k < a; ++k) v -= L[tri(k, a)] * y[k];
        y[a] = v / L[tri(a, a)];
        d2 += y[a] * y[a];
    }
    return ok ? d2 : HUGE_VAL;
}

__global__ __launch_bounds__(256) void pcm_pairs_kernel(const double *prep_a, const double *prep_b, const int *idx_a, const int *idx_b,
                                                         const double *loops, const double *odom, int n, int W, double threshold,
                                                         double *d2, unsigned long long *upper)
{
    const int lane = (int)(threadIdx.x & 63u), w = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
    const int i = (int)blockIdx.y;
    if (w >= W) return;                                    // the whole wave
    const int j = w * 64 + lane;
    const bool act = j > i && j < n;
    double v = HUGE_VAL;
    if (act) v = pair_d2(prep_a, prep_b, idx_a, idx_b, loops, odom, i, j);
    if (d2) {
        if (j == i) d2[(size_t)i * n + i] = 0.0;
        if (act) { d2[(size_t)i * n + j] = v; d2[(size_t)j * n + i] = v; }
    }
    const unsigned long long word = __ballot(act && v <= threshold);          // +inf and NaN: never
    if (lane == 0) upper[(size_t)i * W + w] = word;
}

__global__ __launch_bounds__(64) void pcm_symmetrise_kernel(const unsigned long long *upper, int n, int W, unsigned long long *adj, int *degree)
{
    const int j = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int jw = j >> 6, jb = j & 63;
    int deg = 0;
    for (int w = 0; w < W; ++w) {
        const int i = w * 64 + lane;
        const bool bit = i < j && ((upper[(size_t)i * W + jw] >> jb) & 1ull);
        const unsigned long long word = upper[(size_t)j * W + w] | __ballot(bit);
        if (lane == 0) adj[(size_t)j * W + w] = word;
        deg += __popcll(word);
    }
    if (lane == 0) degree[j] = deg;
}

__device__ inline int wave_max(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
    return v;
}

__device__ inline int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per seed.  P, C and the set X the counts are taken against live as one word per lane (and P, X once more in LDS, where every
// lane reads every word).  cnt[v] = |adj[v] & P| for the v in P, kept from step to step: after u is taken, P' = P & adj[u] and R = P & ~adj[u]
// leave cnt[v] -= |adj[v] & R| -- or cnt[v] = |adj[v] & P'| anew, whichever of R and P' has fewer non-zero words.  Both are the same integer.
// Lane l counts for v = 64 b + l, word b of P after word b, its row read from global memory (the matrix is at most 2 MB: L2).
__global__ __launch_bounds__(64) void pcm_clique_kernel(const unsigned long long *adj, int n, int W, int *best,
                                                         unsigned long long *sets, int *sizes)
{
    __shared__ unsigned long long sP[64], sX[64];
    __shared__ unsigned short cnt[kPcmMaxLoops];
    const int s = (int)blockIdx.x, lane = (int)threadIdx.x;
    unsigned long long P = lane < W ? adj[(size_t)s * W + lane] : 0ull;
    unsigned long long X = P;
    unsigned long long C = lane == (s >> 6) ? 1ull << (s & 63) : 0ull;
    int size = 1;
    // A seed whose degree + 1 is STRICTLY below a clique some seed has finished could not even tie with it: whether this read sees that
    // clique or not changes which seeds run, never the answer.
    const int seen = __builtin_amdgcn_readfirstlane(__atomic_load_n(best, __ATOMIC_RELAXED));
    if (wave_sum(__popcll(P)) + 1 < seen) {
        if (lane == 0) sizes[s] = 0;
        return;
    }
    bool recount = true;
    for (;;) {
        const unsigned long long maskP = __ballot(P != 0ull);
        if (!maskP) break;
        const unsigned long long maskX = __ballot(X != 0ull);
        __syncthreads();
        sP[lane] = P; sX[lane] = X;
        __syncthreads();
        int key = -1;
        for (unsigned long long m = maskP; m; m &= m - 1ull) {
            const int b = __builtin_ctzll(m);
            if ((sP[b] >> lane) & 1ull) {
                const int v = b * 64 + lane;
                const unsigned long long *row = adj + (size_t)v * W;
                int d = 0;
                for (unsigned long long mx = maskX; mx; mx &= mx - 1ull) {
                    const int w = __builtin_ctzll(mx);
                    d += __popcll(row[w] & sX[w]);
                }
                const int c = recount ? d : (int)cnt[v] - d;
                cnt[v] = (unsigned short)c;
                const int k = c * kPcmMaxLoops + (kPcmMaxLoops - 1 - v);      // the largest count, then the lowest index
                key = k > key ? k : key;
            }
        }
        key = wave_max(key);
        const int u = kPcmMaxLoops - 1 - (key & (kPcmMaxLoops - 1));
        const unsigned long long au = lane < W ? adj[(size_t)u * W + lane] : 0ull;
        const unsigned long long R = P & ~au;              // holds u: the diagonal is zero
        P &= au;
        if (lane == (u >> 6)) C |= 1ull << (u & 63);
        ++size;
        recount = __popcll(__ballot(P != 0ull)) <= __popcll(__ballot(R != 0ull));
        X = recount ? P : R;
    }
    if (lane < W) sets[(size_t)s * W + lane] = C;
    if (lane == 0) { sizes[s] = size; atomicMax(best, size); }
}

// result[0] = members, result[1] = seed, result[2 ..] = the members in ascending order
__global__ __launch_bounds__(256) void pcm_clique_finish_kernel(const unsigned long long *sets, const int *sizes, int n, int W, int *result)
{
    __shared__ int red[256];
    __shared__ int offs[64];
    const int tid = (int)threadIdx.x;
    int key = -1;
    for (int s = tid; s < n; s += 256) {
        const int k = sizes[s] * kPcmMaxLoops + (kPcmMaxLoops - 1 - s);        // the largest clique, then the lowest seed
        key = k > key ? k : key;
    }
    red[tid] = key;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = red[tid + o] > red[tid] ? red[tid + o] : red[tid];
        __syncthreads();
    }
    const int win = kPcmMaxLoops - 1 - (red[0] & (kPcmMaxLoops - 1));
    unsigned long long word = 0ull;
    if (tid < 64) { word = tid < W ? sets[(size_t)win * W + tid] : 0ull; offs[tid] = __popcll(word); }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int l = 0; l < 64; ++l) { const int c = offs[l]; offs[l] = run; run += c; }
        result[0] = run; result[1] = win;
    }
    __syncthreads();
    if (tid < 64) {
        int o = offs[tid];
        for (; word; word &= word - 1ull) result[2 + o++] = tid * 64 + __builtin_ctzll(word);
    }
}

#define PCM_HIP(call)                                                                                  \
    do {                                                                                               \
        const hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess) {                                                                       \
            if (err) *err = std::string("pcm: ") + #call + ": " + hipGetErrorString(e__);              \
            return e__ == hipErrorOutOfMemory ? SCL_ERR_NOMEM : SCL_ERR_HIP;                           \
        }                                                                                              \
    } while (0)

int ensure(PcmWorkspace *ws, int k, size_t bytes, std::string *err)
{
    if (bytes <= ws->cap[k]) return SCL_OK;
    if (ws->buf[k]) { (void)hipFree(ws->buf[k]); ws->buf[k] = nullptr; ws->cap[k] = 0; }
    PCM_HIP(hipMalloc(&ws->buf[k], bytes));
    ws->cap[k] = bytes;
    return SCL_OK;
}

template <class T> T *at(PcmWorkspace *ws, int k) { return static_cast<T *>(ws->buf[k]); }

int timing_events(PcmWorkspace *ws, std::string *err)
{
    for (hipEvent_t &ev : ws->ev)
        if (!ev) PCM_HIP(hipEventCreate(&ev));
    return SCL_OK;
}

// the clique of the graph in B_ADJ -> B_RESULT
int enqueue_clique(PcmWorkspace *ws, hipStream_t stream, int n, int W, bool timing, std::string *err)
{
    int rc;
    if ((rc = ensure(ws, PcmWorkspace::B_SETS, sizeof(unsigned long long) * (size_t)n * W, err))) return rc;
    if ((rc = ensure(ws, PcmWorkspace::B_SIZES, sizeof(int) * (size_t)n, err))) return rc;
    if ((rc = ensure(ws, PcmWorkspace::B_BEST, sizeof(int), err))) return rc;
    if ((rc = ensure(ws, PcmWorkspace::B_RESULT, sizeof(int) * ((size_t)n + 2), err))) return rc;
    PCM_HIP(hipMemsetAsync(ws->buf[PcmWorkspace::B_BEST], 0, sizeof(int), stream));
    if (timing) PCM_HIP(hipEventRecord(ws->ev[2], stream));
    pcm_clique_kernel<<<dim3((unsigned)n), dim3(64), 0, stream>>>(at<unsigned long long>(ws, PcmWorkspace::B_ADJ), n, W, at<int>(ws, PcmWorkspace::B_BEST),
                                                                  at<unsigned long long>(ws, PcmWorkspace::B_SETS), at<int>(ws, PcmWorkspace::B_SIZES));
    pcm_clique_finish_kernel<<<dim3(1), dim3(256), 0, stream>>>(at<unsigned long long>(ws, PcmWorkspace::B_SETS), at<int>(ws, PcmWorkspace::B_SIZES), n, W,
                                                                at<int>(ws, PcmWorkspace::B_RESULT));
    PCM_HIP(hipGetLastError());
    if (timing) PCM_HIP(hipEventRecord(ws->ev[3], stream));
    return SCL_OK;
}

int read_clique(PcmWorkspace *ws, hipStream_t stream, int n, int *members, int *n_members, int *seed, std::string *err)
{
    std::vector<int> h((size_t)n + 2);
    PCM_HIP(hipMemcpyAsync(h.data(), ws->buf[PcmWorkspace::B_RESULT], sizeof(int) * h.size(), hipMemcpyDeviceToHost, stream));
    PCM_HIP(hipStreamSynchronize(stream));
    if (h[0] < 1 || h[0] > n || h[1] < 0 || h[1] >= n) { if (err) *err = "pcm: the clique kernel left no result"; return SCL_ERR_HIP; }
    std::memcpy(members, h.data() + 2, sizeof(int) * (size_t)h[0]);
    *n_members = h[0];
    *seed = h[1];
    return SCL_OK;
}

int read_timing(PcmWorkspace *ws, bool pairs, bool clique, std::string *err)
{
    float ms = 0.f;
    ws->pairs_ms = ws->clique_ms = 0.0;
    if (pairs) { PCM_HIP(hipEventElapsedTime(&ms, ws->ev[0], ws->ev[1])); ws->pairs_ms = ms; }
    if (clique) { PCM_HIP(hipEventElapsedTime(&ms, ws->ev[2], ws->ev[3])); ws->clique_ms = ms; }
    return SCL_OK;
}

bool finite_all(const double *p, size_t n)
{
    for (size_t k = 0; k < n; ++k) if (!std::isfinite(p[k])) return false;
    return true;
}

bool quaternions_ok(const double *poses, int n)
{
    for (int k = 0; k < n; ++k) {
        const double *q = poses + 7 * (size_t)k + 3;
        const double s = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        if (!(s >= 0.25 && s <= 4.0)) return false;
    }
    return true;
}

}  // namespace

void pcm_workspace_free(PcmWorkspace *ws)
{
    for (int k = 0; k < PcmWorkspace::B_COUNT; ++k) {
        if (ws->buf[k]) (void)hipFree(ws->buf[k]);
        ws->buf[k] = nullptr; ws->cap[k] = 0;
    }
    for (hipEvent_t &ev : ws->ev) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
}

const char *pcm_inputs_bad(const PcmInputs &in)
{
    if (in.n_a < 0 || in.n_b < 0 || in.n_loops < 0) return "a negative count";
    if (in.n_loops > kPcmMaxLoops) return "more than 4096 loops";
    if ((in.n_a > 0 && !in.poses_a) || (in.n_b > 0 && !in.poses_b)) return "poses == NULL";
    if (in.n_loops > 0 && (!in.idx_a || !in.idx_b || !in.z || !in.cov)) return "a loop array is NULL";
    if (!std::isfinite(in.threshold) || in.threshold < 0.0) return "threshold non-finite or negative";
    if (in.odom_var)
        for (int k = 0; k < 6; ++k) if (!std::isfinite(in.odom_var[k]) || in.odom_var[k] < 0.0) return "odom_var non-finite or negative";
    for (int i = 0; i < in.n_loops; ++i)
        if (in.idx_a[i] < 0 || in.idx_a[i] >= in.n_a || in.idx_b[i] < 0 || in.idx_b[i] >= in.n_b) return "a keyframe index out of range";
    if (!finite_all(in.poses_a, 7 * (size_t)in.n_a) || !finite_all(in.poses_b, 7 * (size_t)in.n_b) || !finite_all(in.z, 7 * (size_t)in.n_loops))
        return "a non-finite pose";
    for (int i = 0; i < in.n_loops; ++i)
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) if (!std::isfinite(in.cov[36 * (size_t)i + 6 * a + b])) return "a non-finite covariance";
    if (!quaternions_ok(in.poses_a, in.n_a) || !quaternions_ok(in.poses_b, in.n_b) || !quaternions_ok(in.z, in.n_loops))
        return "a quaternion's squared norm outside [0.25, 4]";
    return nullptr;
}

const char *pcm_graph_bad(const uint64_t *adj, int n)
{
    if (n < 0) return "a negative count";
    if (n > kPcmMaxLoops) return "more than 4096 vertices";
    if (n > 0 && !adj) return "adj == NULL";
    const int W = (n + 63) / 64;
    for (int i = 0; i < n; ++i)
        for (int w = 0; w < W; ++w)
            for (uint64_t m = adj[(size_t)i * W + w]; m; m &= m - 1) {
                const int j = w * 64 + __builtin_ctzll(m);
                if (j >= n) return "a bit at or beyond n";
                if (j == i) return "a diagonal bit";
                if (!((adj[(size_t)j * W + (i >> 6)] >> (i & 63)) & 1u)) return "adj is not symmetric";
            }
    return nullptr;
}

int pcm_consistency(PcmWorkspace *ws, hipStream_t stream, const PcmInputs &in, double *d2, uint64_t *adj, int *degree,
                    int *members, int *n_members, int *seed, bool timing, std::string *err)
{
    using WS = PcmWorkspace;
    const int n = in.n_loops, W = (n + 63) / 64;
    const size_t na = (size_t)in.n_a, nb = (size_t)in.n_b, nn = (size_t)n;
    int rc;
    if ((rc = ensure(ws, WS::B_POSES_A, sizeof(double) * 7 * na, err)) || (rc = ensure(ws, WS::B_POSES_B, sizeof(double) * 7 * nb, err)) ||
        (rc = ensure(ws, WS::B_IDX_A, sizeof(int) * nn, err)) || (rc = ensure(ws, WS::B_IDX_B, sizeof(int) * nn, err)) ||
        (rc = ensure(ws, WS::B_Z, sizeof(double) * 7 * nn, err)) || (rc = ensure(ws, WS::B_COV, sizeof(double) * 36 * nn, err)) ||
        (rc = ensure(ws, WS::B_ODOM, sizeof(double) * 6, err)) ||
        (rc = ensure(ws, WS::B_PREP_A, sizeof(double) * kPoseStride * na, err)) || (rc = ensure(ws, WS::B_PREP_B, sizeof(double) * kPoseStride * nb, err)) ||
        (rc = ensure(ws, WS::B_LOOPS, sizeof(double) * kLoopStride * nn, err)) ||
        (rc = ensure(ws, WS::B_UPPER, sizeof(unsigned long long) * nn * W, err)) || (rc = ensure(ws, WS::B_ADJ, sizeof(unsigned long long) * nn * W, err)) ||
        (rc = ensure(ws, WS::B_DEGREE, sizeof(int) * nn, err)))
        return rc;
    if (d2 && (rc = ensure(ws, WS::B_D2, sizeof(double) * nn * nn, err))) return rc;
    if (timing && (rc = timing_events(ws, err))) return rc;
    const double zeros[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    PCM_HIP(hipMemcpyAsync(ws->buf[WS::B_POSES_A], in.poses_a, sizeof(double) * 7 * na, hipMemcpyHostToDevice, stream));
    PCM_HIP(hipMemcpyAsync(ws->buf[WS::B_POSES_B], in.poses_b, sizeof(double) * 7 * nb, hipMemcpyHostToDevice, stream));
    PCM_HIP(hipMemcpyAsync(ws->buf[WS::B_IDX_A], in.idx_a, sizeof(int) * nn, hipMemcpyHostToDevice, stream));
    PCM_HIP(hipMemcpyAsync(ws->buf[WS::B_IDX_B], in.idx_b, sizeof(int) * nn, hipMemcpyHostToDevice, stream));
    PCM_HIP(hipMemcpyAsync(ws->buf[WS::B_Z], in.z, sizeof(double) * 7 * nn, hipMemcpyHostToDevice, stream));
    PCM_HIP(hipMemcpyAsync(ws->buf[WS::B_COV], in.cov, sizeof(double) * 36 * nn, hipMemcpyHostToDevice, stream));
    PCM_HIP(hipMemcpyAsync(ws->buf[WS::B_ODOM], in.odom_var ? in.odom_var : zeros, sizeof(double) * 6, hipMemcpyHostToDevice, stream));
    PCM_HIP(hipStreamSynchronize(stream));                 // `zeros` and the caller's arrays are pageable: nothing of them is read after this
    if (timing) PCM_HIP(hipEventRecord(ws->ev[0], stream));
    const size_t items = na + nb + nn;
    pcm_prep_kernel<<<dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream>>>(
        at<double>(ws, WS::B_POSES_A), in.n_a, at<double>(ws, WS::B_POSES_B), in.n_b, at<double>(ws, WS::B_Z), at<double>(ws, WS::B_COV), n,
        at<double>(ws, WS::B_PREP_A), at<double>(ws, WS::B_PREP_B), at<double>(ws, WS::B_LOOPS));
    pcm_pairs_kernel<<<dim3((unsigned)((W + 3) / 4), (unsigned)n), dim3(256), 0, stream>>>(
        at<double>(ws, WS::B_PREP_A), at<double>(ws, WS::B_PREP_B), at<int>(ws, WS::B_IDX_A), at<int>(ws, WS::B_IDX_B), at<double>(ws, WS::B_LOOPS),
        at<double>(ws, WS::B_ODOM), n, W, in.threshold, d2 ? at<double>(ws, WS::B_D2) : nullptr, at<unsigned long long>(ws, WS::B_UPPER));
    pcm_symmetrise_kernel<<<dim3((unsigned)n), dim3(64), 0, stream>>>(at<unsigned long long>(ws, WS::B_UPPER), n, W,
                                                                      at<unsigned long long>(ws, WS::B_ADJ), at<int>(ws, WS::B_DEGREE));
    PCM_HIP(hipGetLastError());
    if (timing) PCM_HIP(hipEventRecord(ws->ev[1], stream));
    if (members && (rc = enqueue_clique(ws, stream, n, W, timing, err))) return rc;
    // read everything into the caller's arrays only once the whole call has run
    if (d2) PCM_HIP(hipMemcpyAsync(d2, ws->buf[WS::B_D2], sizeof(double) * nn * nn, hipMemcpyDeviceToHost, stream));
    if (adj) PCM_HIP(hipMemcpyAsync(adj, ws->buf[WS::B_ADJ], sizeof(unsigned long long) * nn * W, hipMemcpyDeviceToHost, stream));
    if (degree) PCM_HIP(hipMemcpyAsync(degree, ws->buf[WS::B_DEGREE], sizeof(int) * nn, hipMemcpyDeviceToHost, stream));
    if (members) { if ((rc = read_clique(ws, stream, n, members, n_members, seed, err))) return rc; }
    else PCM_HIP(hipStreamSynchronize(stream));
    if (timing) return read_timing(ws, true, members != nullptr, err);
    return SCL_OK;
}

int pcm_max_clique(PcmWorkspace *ws, hipStream_t stream, const uint64_t *adj, int n, int *members, int *n_members, int *seed,
                   bool timing, std::string *err)
{
    const int W = (n + 63) / 64;
    int rc;
    if ((rc = ensure(ws, PcmWorkspace::B_ADJ, sizeof(unsigned long long) * (size_t)n * W, err))) return rc;
    if (timing && (rc = timing_events(ws, err))) return rc;
    PCM_HIP(hipMemcpyAsync(ws->buf[PcmWorkspace::B_ADJ], adj, sizeof(unsigned long long) * (size_t)n * W, hipMemcpyHostToDevice, stream));
    PCM_HIP(hipStreamSynchronize(stream));
    if ((rc = enqueue_clique(ws, stream, n, W, timing, err))) return rc;
    if ((rc = read_clique(ws, stream, n, members, n_members, seed, err))) return rc;
    if (timing) return read_timing(ws, false, true, err);
    return SCL_OK;
}

}  // namespace scl
