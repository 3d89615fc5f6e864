// se3_device.hpp -- the fp64 quaternion, composition and adjoint helpers the SE(3) kernels share (pcm.hip, pgo.hip).  A pose on the
// device is 8 doubles: the unit quaternion (x, y, z, w), the translation, one pad.  Every function is one fixed sequence of operations;
// the build forbids contraction, so both files get the same bits from them.
#pragma once

#include <hip/hip_runtime.h>

namespace scl {
namespace se3 {

constexpr int kPoseStride = 8;     // q (x, y, z, w) normalised, t, one pad

// index of (a, b), a <= b, in the row-by-row upper triangle of a 6 x 6
__host__ __device__ constexpr int tri(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }

// Hamilton product of (x, y, z, w) quaternions: R(a * b) = R(a) R(b)
__device__ inline void qmul(const double *a, const double *b, double *o)
{
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}

__device__ inline void qconj(const double *a, double *o) { o[0] = -a[0]; o[1] = -a[1]; o[2] = -a[2]; o[3] = a[3]; }

// R(q) v for a unit q: v + w c + u x c with c = 2 u x v
__device__ inline void qrot(const double *q, const double *v, double *o)
{
    const double cx = 2.0 * (q[1] * v[2] - q[2] * v[1]), cy = 2.0 * (q[2] * v[0] - q[0] * v[2]), cz = 2.0 * (q[0] * v[1] - q[1] * v[0]);
    o[0] = v[0] + q[3] * cx + (q[1] * cz - q[2] * cy);
    o[1] = v[1] + q[3] * cy + (q[2] * cx - q[0] * cz);
    o[2] = v[2] + q[3] * cz + (q[0] * cy - q[1] * cx);
}

// the rotation matrix of a unit q, row major
__device__ inline void qmat(const double *q, double *R)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - z * w);       R[2] = 2.0 * (x * z + y * w);
    R[3] = 2.0 * (x * y + z * w);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - x * w);
    R[6] = 2.0 * (x * z - y * w);       R[7] = 2.0 * (y * z + x * w);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

__device__ inline void mm(const double *A, const double *B, double *C)        // C = A B
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}

__device__ inline void mmt(const double *A, const double *B, double *C)       // C = A B^T
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1] + A[3 * r + 2] * B[3 * c + 2];
}

// the blocks of Ad(q, t) = [[R, 0], [B, R]]: R = R(q), B = [t]x R
__device__ inline void adjoint_blocks(const double *q, const double *t, double *R, double *B)
{
    qmat(q, R);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        B[c]     = t[1] * R[6 + c] - t[2] * R[3 + c];
        B[3 + c] = t[2] * R[c] - t[0] * R[6 + c];
        B[6 + c] = t[0] * R[3 + c] - t[1] * R[c];
    }
}

// a pose of the interface (x, y, z, qx, qy, qz, qw) -> q normalised in double, t
__device__ inline void normalise_pose(const double *in, double *out)
{
    const double s = sqrt(in[3] * in[3] + in[4] * in[4] + in[5] * in[5] + in[6] * in[6]);
    out[0] = in[3] / s; out[1] = in[4] / s; out[2] = in[5] / s; out[3] = in[6] / s;
    out[4] = in[0]; out[5] = in[1]; out[6] = in[2];
}

// (X_from)^-1 X_to of two prepared poses: q = conj(q_from) q_to, t = R(q_from)^T (t_to - t_from) -- the difference first, so that a
// trajectory far from its origin costs nothing
__device__ inline void relative_pose(const double *from, const double *to, double *q, double *t)
{
    double c[4];
    qconj(from, c);
    qmul(c, to, q);
    const double d[3] = {to[4] - from[4], to[5] - from[5], to[6] - from[6]};
    qrot(c, d, t);
}

// (q1, t1) (q2, t2)
__device__ inline void compose(const double *q1, const double *t1, const double *q2, const double *t2, double *q, double *t)
{
    double r[3];
    qmul(q1, q2, q);
    qrot(q1, t2, r);
    t[0] = t1[0] + r[0]; t[1] = t1[1] + r[1]; t[2] = t1[2] + r[2];
}

// Log_SO3 of a unit quaternion, w made >= 0: 2 atan2(|v|, w) v / |v|, and 2 v where |v| = 0.  qp = the quaternion with w >= 0, *nv = |v|
__device__ inline void qlog(const double *q, double *w3, double *qp, double *nv)
{
    const double sg = q[3] < 0.0 ? -1.0 : 1.0;
    const double x = sg * q[0], y = sg * q[1], zc = sg * q[2], w = sg * q[3];
    const double n = sqrt(x * x + y * y + zc * zc);
    const double k = n == 0.0 ? 2.0 : 2.0 * atan2(n, w) / n;
    w3[0] = k * x; w3[1] = k * y; w3[2] = k * zc;
    qp[0] = x; qp[1] = y; qp[2] = zc; qp[3] = w;
    *nv = n;
}

}  // namespace se3
}  // namespace scl
