// Pose-graph optimisation (include/nof.h group 9): Gauss-Newton over the poses of a window of frames,
// a Huber-robust point-to-point term over sparse 3-D matches plus a Huber-robust projective
// point-to-plane term between every overlapping pair of point/normal maps, an inner preconditioned
// conjugate-gradient solve per outer iteration. The reference's counterpart is CUDASolverBundling
// (BundleTrack/src/cuda/Solver/SolverBundling.cu) in float32 with float atomics; here every sum is
// f64 in a fixed order, nothing is decided on the host inside the loop and a run repeats bit for bit.
//
// Definition (all f64, no contraction; (x + y) + z means that order of additions).
//  State. Poses are 4x4 camera-in-world matrices T_k = [R_k | t_k]. The variables of frame k are
//    delta_k = [omega, v], rotation first; the update is T_k <- Exp(delta_k) T_k. Exp: th2 =
//    (wx wx + wy wy) + wz wz, cr = omega x v. th2 < 1e-8: A = 1 - th2/6, B = 0.5, t = v + 0.5 cr.
//    Else th2 < 1e-6: C = (1 - th2/20)/6, A = 1 - th2 C, B = 0.5 - th2/24; otherwise th = sqrt(th2),
//    A = sin(th)/th, B = (1 - cos(th))/th2, C = (1 - A)/th2; t = (v + B cr) + C (omega x cr). R = I +
//    A [omega]x + B [omega]x^2 written out per entry (exp_se3 below). The product row r, column c is
//    (E[r][0] T[0][c] + E[r][1] T[1][c]) + E[r][2] T[2][c], plus E[r][3] for c = 3. A fixed frame is
//    a constant: its pose comes back bit for bit and its rows and columns of the system are zero.
//  Point transform. (T p)_k = ((T[k][0] px + T[k][1] py) + T[k][2] pz) + T[k][3]; a normal is
//    rotated the same way without the last term (xform_point / xform_dir of geom_device.h, which also
//    holds the block sum of the kernels below and pair_rows).
//  Huber. For a squared residual e and delta: e <= delta^2: rho = e, rho' = 1; else s = sqrt(e),
//    rho = 2 s delta - delta^2, rho' = delta / s.
//  Sparse row of pair (i, j), match (pa, pb), weight wt (a row with wt == 0 does not exist).
//    a = T_i pa, b = T_j pb, r = a - b, e = (r0 r0 + r1 r1) + r2 r2, w = (w_sparse wt) rho'.
//    Ja = [-[a]x | I], Jb = [-[b]x | I] (3x6; J_i = Ja, J_j = -Jb). With dot(x, y) =
//    (x0 y0 + x1 y1) + x2 y2 over the three rows: A_ii[r][c] += w dot(Ja_r, Ja_c), A_jj += w dot(Jb_r,
//    Jb_c), X[r][c] += w dot(Ja_r, Jb_c) (A_ij = -X, A_ji = -X^T), hi[r] += w dot(Ja_r, r), hj[r] +=
//    w dot(Jb_r, r) (g_i -= hi, g_j += hj). Energy += (w_sparse wt) rho, live rows += 1.
//  Dense pairs. A point of a map is valid if depth_min < z < depth_max and its normal is not all
//    zero. The unordered pair {lo < hi} is taken once: the source j is the frame with fewer valid
//    points, hi on a tie; the target i is the other. Rij = R_i^T R_j entry (r, c) = (Ri[0][r]
//    Rj[0][c] + Ri[1][r] Rj[1][c]) + Ri[2][r] Rj[2][c], tij[r] = (Ri[0][r] d0 + Ri[1][r] d1) + Ri[2][r]
//    d2 with d = t_j - t_i. The pair is active iff (Rij00 + Rij11) + Rij22 > min_trace (= 1 + 2
//    cos(max_rot): the geodesic angle is below max_rot).
//  Dense correspondence of a valid source pixel s: q = Rij ps + tij, nq = Rij ns. None unless qz > 0.
//    u = (fx qx) / qz + cx, v = (fy qy) / qz + cy, w0 = round(u), h0 = round(v) (halves away from
//    zero); none if |u| or |v| >= 1e9. The window h0-radius .. h0+radius by w0-radius .. w0+radius is
//    scanned row-major inside the image. A candidate t qualifies if it is valid, dist = sqrt((dx dx +
//    dy dy) + dz dz) <= dist_thresh with dx = ptx - qx, and dn = (nqx ntx + nqy nty) + nqz ntz >=
//    normal_thresh; score = (1 - dn) + dist / dist_thresh, the lowest wins, the first of equals.
//  Dense row. d = (ntx dx + nty dy) + ntz dz, e = d d, w = w_dense rho'. a = T_j ps, m = R_i nt, u =
//    [a x m, m] with (a x m)_0 = ay mz - az my and cyclic. J_i = +u, J_j = -u. S[r][c] += (w u_r) u_c
//    for r <= c, h[r] += (w u_r) d: A_ii += S, A_jj += S, A_ij = A_ji -= S, g_i -= h, g_j += h.
//    Energy += w_dense rho, correspondences += 1.
//  System. A = sum w J^T J, g = -sum w J^T r over all rows; the Huber weight is in both.
//  Solve. n_inner steps of PCG from delta = 0: Minv[r] = 1 / A[r][r] if A[r][r] > 1e-6 else 1; r = g,
//    z = Minv r, p = z, rz = r.z; per step Ap = A p (row r: columns added in ascending order), pAp =
//    p.Ap, alpha = rz / pAp if pAp > 1e-6 else 0, delta += alpha p, r -= alpha Ap, z = Minv r, rz' =
//    z.r, beta = rz' / rz if rz > 1e-6 else 0, p = z + beta p, rz = rz'. A dot product: thread t of
//    256 adds its rows t, t + 256, ... in order, a butterfly (xor 32, 16, .. 1) adds the lanes of a
//    wave, the four waves are added in order.
//
//  k_pg_prepare   a block per frame: the working copy of the pose, the frame's valid-point count.
//  k_pg_sparse    a block per (pair, chunk): walks every gridDim.x-th tile of 256 rows of the pair; a
//                 lane adds its rows in order, lanes meet by butterfly, waves through LDS in order;
//                 the 92 partials of the (pair, chunk) go to the workspace.
//  k_pg_dense     the hot kernel, a block per (lo, hi, chunk): a lane owns a source pixel and its
//                 window search and keeps 21 + 6 + 2 sums; an inactive pair writes zeros and leaves.
//  k_pg_assemble  a block per 6x6 block of A: pair partials in pair order, chunks in order, sparse
//                 first, then the dense pairs in the order of the other frame; one more block adds
//                 the energies and counts. The second pass of every cross-block sum.
//  k_pg_solve     one block: PCG on the explicit A, the Lie update, the history row.
#include <math.h>

#include "geom_device.h"
#include "host_entry.h"

#pragma clang fp contract(off)

namespace nof {

constexpr int PG_MAX_FRAMES = 128;
constexpr int PG_MAX_VARS = 6 * PG_MAX_FRAMES;
constexpr int PG_TILE = 256;            // rows or pixels a block takes at a time: one per thread
constexpr int PG_SP = 92;               // 21 A_ii + 21 A_jj + 36 X + 6 hi + 6 hj + energy + rows
constexpr int PG_DN = 29;               // 21 S + 6 h + energy + correspondences
constexpr int PG_SP_MAX_CHUNKS = 8;
constexpr int PG_DN_MAX_CHUNKS = 32;
constexpr int PG_MAX_RADIUS = 32;
constexpr double PG_EPS = 1e-6;         // FLOAT_EPSILON of the reference's PCG guards

// index of (r, c), r <= c, in the 21 entries of a symmetric 6x6
__host__ __device__ constexpr int pg_sym(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }
__device__ __forceinline__ int pg_sym_any(int r, int c) { return r <= c ? pg_sym(r, c) : pg_sym(c, r); }

__device__ __forceinline__ void pg_huber(double e, double delta, double &rho, double &drho) {
    if (e <= delta * delta) {
        rho = e;
        drho = 1.0;
    } else {
        const double s = sqrt(e);
        rho = (2.0 * s) * delta - delta * delta;
        drho = delta / s;
    }
}

// [-[a]x | I]: the Jacobian of Exp(delta) a at delta = 0
__device__ __forceinline__ void pg_jac(const double (&a)[3], double (&J)[3][6]) {
    J[0][0] = 0.0;   J[0][1] = a[2];  J[0][2] = -a[1];
    J[1][0] = -a[2]; J[1][1] = 0.0;   J[1][2] = a[0];
    J[2][0] = a[1];  J[2][1] = -a[0]; J[2][2] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) J[k][3 + c] = k == c ? 1.0 : 0.0;
}

__device__ __forceinline__ bool pg_valid(const float *__restrict__ p, const float *__restrict__ n, double depth_min,
                                         double depth_max) {
    const double z = (double)p[2];
    return z > depth_min && z < depth_max && !(n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f);
}

__global__ __launch_bounds__(256) void k_pg_prepare(const double *__restrict__ poses, int32_t N,
                                                    const float *__restrict__ points,
                                                    const float *__restrict__ normals, int32_t HW, double depth_min,
                                                    double depth_max, double *__restrict__ T,
                                                    int32_t *__restrict__ cnt, double *__restrict__ iter_poses) {
    __shared__ int32_t wave_cnt[4];
    const int32_t f = blockIdx.x;
    if (threadIdx.x < 16) {
        const double v = poses[(size_t)f * 16 + threadIdx.x];
        T[(size_t)f * 16 + threadIdx.x] = v;
        if (iter_poses) iter_poses[(size_t)f * 16 + threadIdx.x] = v;
    }
    int32_t c = 0;
    if (points) {
        const float *P = points + (size_t)f * HW * 3, *Nn = normals + (size_t)f * HW * 3;
        for (int32_t s = threadIdx.x; s < HW; s += 256) c += pg_valid(P + (size_t)s * 3, Nn + (size_t)s * 3, depth_min, depth_max) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) cnt[f] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

__global__ __launch_bounds__(256) void k_pg_sparse(const int32_t *__restrict__ pair_frames,
                                                   const double *__restrict__ pts_a, const double *__restrict__ pts_b,
                                                   const int32_t *__restrict__ pair_start,
                                                   const double *__restrict__ weight, int64_t M, int32_t N,
                                                   const double *__restrict__ T, double delta, double w_sparse,
                                                   double *__restrict__ part) {
    __shared__ double wave_sum[4][PG_SP];
    const int32_t p = blockIdx.y;
    const int32_t i = pair_frames[p * 2], j = pair_frames[p * 2 + 1];
    double *out = part + ((size_t)p * gridDim.x + blockIdx.x) * PG_SP;
    if (i < 0 || i >= N || j < 0 || j >= N || i == j) {          // no such pair: zeros, so assemble may add them
        if (threadIdx.x < PG_SP) out[threadIdx.x] = 0.0;
        return;
    }
    int64_t s;
    int32_t n;
    pair_rows(pair_start, p, M, s, n);
    const double *Ti = T + (size_t)i * 16, *Tj = T + (size_t)j * 16;
    double acc[PG_SP];
#pragma unroll
    for (int k = 0; k < PG_SP; ++k) acc[k] = 0.0;
    const int32_t n_tiles = (n + PG_TILE - 1) / PG_TILE;
    for (int32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int32_t row = tile * PG_TILE + threadIdx.x;
        if (row >= n) continue;
        const size_t m = (size_t)(s + row);                      // inside [0, M)
        const double wt = weight ? weight[m] : 1.0;
        if (wt == 0.0) continue;
        double a[3], b[3], r[3];
        xform_point(Ti, pts_a[m * 3], pts_a[m * 3 + 1], pts_a[m * 3 + 2], a);
        xform_point(Tj, pts_b[m * 3], pts_b[m * 3 + 1], pts_b[m * 3 + 2], b);
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = a[k] - b[k];
        const double e = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
        double rho, drho;
        pg_huber(e, delta, rho, drho);
        const double w0 = w_sparse * wt, w = w0 * drho;
        double Ja[3][6], Jb[3][6];
        pg_jac(a, Ja);
        pg_jac(b, Jb);
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) {
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                if (c >= rr) {
                    acc[pg_sym(rr, c)] += w * ((Ja[0][rr] * Ja[0][c] + Ja[1][rr] * Ja[1][c]) + Ja[2][rr] * Ja[2][c]);
                    acc[21 + pg_sym(rr, c)] += w * ((Jb[0][rr] * Jb[0][c] + Jb[1][rr] * Jb[1][c]) + Jb[2][rr] * Jb[2][c]);
                }
                acc[42 + rr * 6 + c] += w * ((Ja[0][rr] * Jb[0][c] + Ja[1][rr] * Jb[1][c]) + Ja[2][rr] * Jb[2][c]);
            }
            acc[78 + rr] += w * ((Ja[0][rr] * r[0] + Ja[1][rr] * r[1]) + Ja[2][rr] * r[2]);
            acc[84 + rr] += w * ((Jb[0][rr] * r[0] + Jb[1][rr] * r[1]) + Jb[2][rr] * r[2]);
        }
        acc[90] += w0 * rho;
        acc[91] += 1.0;
    }
    block_sum<PG_SP>(acc, wave_sum, out);
}

struct PgDense {
    const float *points, *normals;     // [N,H,W,3]
    int32_t N, H, W, radius;
    double fx, fy, cx, cy;
    double delta, w_dense, dist_thresh, normal_thresh, depth_min, depth_max, min_trace;
};

// The target of the unordered pair lo < hi: the source is the frame with fewer valid points, hi on a tie.
__device__ __forceinline__ int32_t pg_dense_target(const int32_t *__restrict__ cnt, int32_t lo, int32_t hi) {
    return cnt[hi] <= cnt[lo] ? lo : hi;
}

__global__ __launch_bounds__(256) void k_pg_dense(PgDense d, const double *__restrict__ T,
                                                  const int32_t *__restrict__ cnt, double *__restrict__ part,
                                                  int32_t *__restrict__ dense_index) {
    __shared__ double rel[12];
    __shared__ double wave_sum[4][PG_DN];
    const int32_t lo = blockIdx.z, hi = blockIdx.y;
    if (lo >= hi) return;                                        // the unordered pair is taken once
    const int32_t i = pg_dense_target(cnt, lo, hi), j = i == lo ? hi : lo;
    const double *Ti = T + (size_t)i * 16, *Tj = T + (size_t)j * 16;
    if (threadIdx.x < 12) {
        const int r = threadIdx.x >> 2, c = threadIdx.x & 3;
        double v;
        if (c < 3) {
            v = (Ti[r] * Tj[c] + Ti[4 + r] * Tj[4 + c]) + Ti[8 + r] * Tj[8 + c];
        } else {
            const double d0 = Tj[3] - Ti[3], d1 = Tj[7] - Ti[7], d2 = Tj[11] - Ti[11];
            v = (Ti[r] * d0 + Ti[4 + r] * d1) + Ti[8 + r] * d2;
        }
        rel[threadIdx.x] = v;
    }
    __syncthreads();
    const int32_t slot = hi * (hi - 1) / 2 + lo;
    double *out = part + ((size_t)slot * gridDim.x + blockIdx.x) * PG_DN;
    const bool active = (rel[0] + rel[5]) + rel[10] > d.min_trace;      // false for NaN poses
    if (!active) {
        if (threadIdx.x < PG_DN) out[threadIdx.x] = 0.0;
        return;
    }
    const int32_t HW = d.H * d.W;
    const float *Pt = d.points + (size_t)i * HW * 3, *Nt = d.normals + (size_t)i * HW * 3;
    const float *Ps = d.points + (size_t)j * HW * 3, *Ns = d.normals + (size_t)j * HW * 3;
    int32_t *index = dense_index ? dense_index + ((size_t)i * d.N + j) * HW : nullptr;
    double acc[PG_DN];
#pragma unroll
    for (int k = 0; k < PG_DN; ++k) acc[k] = 0.0;
    const int32_t n_tiles = (HW + PG_TILE - 1) / PG_TILE;
    for (int32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int32_t s = tile * PG_TILE + threadIdx.x;
        if (s >= HW) continue;
        int32_t best = -1;
        double q[3] = {0.0, 0.0, 0.0};
        const double px = (double)Ps[(size_t)s * 3], py = (double)Ps[(size_t)s * 3 + 1], pz = (double)Ps[(size_t)s * 3 + 2];
        if (pg_valid(Ps + (size_t)s * 3, Ns + (size_t)s * 3, d.depth_min, d.depth_max)) {
            const double nx = (double)Ns[(size_t)s * 3], ny = (double)Ns[(size_t)s * 3 + 1], nz = (double)Ns[(size_t)s * 3 + 2];
            double nq[3];
            xform_point(rel, px, py, pz, q);
            xform_dir(rel, nx, ny, nz, nq);
            if (q[2] > 0.0) {
                const double u = (d.fx * q[0]) / q[2] + d.cx, v = (d.fy * q[1]) / q[2] + d.cy;
                if (fabs(u) < 1e9 && fabs(v) < 1e9) {                    // false for NaN
                    const int32_t w0 = (int32_t)round(u), h0 = (int32_t)round(v);
                    const int32_t hA = h0 - d.radius < 0 ? 0 : h0 - d.radius;
                    const int32_t hB = h0 + d.radius > d.H - 1 ? d.H - 1 : h0 + d.radius;
                    const int32_t wA = w0 - d.radius < 0 ? 0 : w0 - d.radius;
                    const int32_t wB = w0 + d.radius > d.W - 1 ? d.W - 1 : w0 + d.radius;
                    double best_score = INFINITY;
                    for (int32_t h = hA; h <= hB; ++h) {
                        for (int32_t w = wA; w <= wB; ++w) {
                            const int32_t t = h * d.W + w;               // inside the image: 0 <= t < HW
                            const float *pt = Pt + (size_t)t * 3, *nt = Nt + (size_t)t * 3;
                            if (!pg_valid(pt, nt, d.depth_min, d.depth_max)) continue;
                            const double dx = (double)pt[0] - q[0], dy = (double)pt[1] - q[1], dz = (double)pt[2] - q[2];
                            const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
                            if (!(dist <= d.dist_thresh)) continue;
                            const double dn = (nq[0] * (double)nt[0] + nq[1] * (double)nt[1]) + nq[2] * (double)nt[2];
                            if (!(dn >= d.normal_thresh)) continue;
                            const double score = (1.0 - dn) + dist / d.dist_thresh;
                            if (score < best_score) {
                                best_score = score;
                                best = t;
                            }
                        }
                    }
                }
            }
        }
        if (index) index[s] = best;
        if (best < 0) continue;
        const float *pt = Pt + (size_t)best * 3, *nt = Nt + (size_t)best * 3;
        const double ntx = (double)nt[0], nty = (double)nt[1], ntz = (double)nt[2];
        const double dx = (double)pt[0] - q[0], dy = (double)pt[1] - q[1], dz = (double)pt[2] - q[2];
        const double res = (ntx * dx + nty * dy) + ntz * dz;
        double rho, drho;
        pg_huber(res * res, d.delta, rho, drho);
        const double w = d.w_dense * drho;
        double a[3], u[6];
        xform_point(Tj, px, py, pz, a);
        xform_dir(Ti, ntx, nty, ntz, u + 3);
        u[0] = a[1] * u[5] - a[2] * u[4];
        u[1] = a[2] * u[3] - a[0] * u[5];
        u[2] = a[0] * u[4] - a[1] * u[3];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const double wu = w * u[r];
#pragma unroll
            for (int c = r; c < 6; ++c) acc[pg_sym(r, c)] += wu * u[c];
            acc[21 + r] += wu * res;
        }
        acc[27] += d.w_dense * rho;
        acc[28] += 1.0;
    }
    block_sum<PG_DN>(acc, wave_sum, out);
}

struct PgAssemble {
    const int32_t *pair_frames;        // [P,2] or NULL
    const uint8_t *fixed;              // [N]
    const int32_t *cnt;                // [N]
    const double *sp_part, *dn_part;
    int32_t N, P, sp_chunks, dn_chunks;     // dn_chunks 0: no dense term
};

// Blocks 0 .. N N - 1: the 6x6 block (bi, bj) of A and, on the diagonal, the 6 entries of g. Block N N
// (the only one of a totals-only launch): the four history sums.
__global__ __launch_bounds__(256) void k_pg_assemble(PgAssemble d, int32_t totals_only, double *__restrict__ A,
                                                     double *__restrict__ g, double *__restrict__ totals,
                                                     double *__restrict__ dbg_A, double *__restrict__ dbg_g) {
    const int32_t N = d.N, n = 6 * N;
    const int32_t n_slots = N * (N - 1) / 2;
    if (totals_only || (int32_t)blockIdx.x == N * N) {
        __shared__ double wave_sum[4][4];
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int32_t p = threadIdx.x; p < d.P; p += 256)
            for (int32_t c = 0; c < d.sp_chunks; ++c) {
                const double *q = d.sp_part + ((size_t)p * d.sp_chunks + c) * PG_SP;
                acc[0] += q[90];
                acc[2] += q[91];
            }
        if (d.dn_chunks)
            for (int32_t s = threadIdx.x; s < n_slots; s += 256)
                for (int32_t c = 0; c < d.dn_chunks; ++c) {
                    const double *q = d.dn_part + ((size_t)s * d.dn_chunks + c) * PG_DN;
                    acc[1] += q[27];
                    acc[3] += q[28];
                }
        block_sum<4>(acc, wave_sum, totals);
        return;
    }
    const int32_t bi = blockIdx.x / N, bj = blockIdx.x % N;
    const int t = threadIdx.x;
    const bool is_g = t >= 36;
    if (t >= 42 || (is_g && bi != bj)) return;
    const int r = is_g ? t - 36 : t / 6, c = is_g ? 0 : t % 6;
    double acc = 0.0;
    if (!d.fixed[bi] && !d.fixed[bj]) {
        for (int32_t p = 0; p < d.P; ++p) {
            const int32_t i = d.pair_frames[p * 2], j = d.pair_frames[p * 2 + 1];
            if (i == j || (i != bi && j != bi)) continue;        // a pair kernel k_pg_sparse refused has zeros anyway
            int off;
            bool neg;
            if (is_g) {
                off = i == bi ? 78 + r : 84 + r;                  // g_i -= hi, g_j += hj
                neg = i == bi;
            } else if (bi == bj) {
                off = (i == bi ? 0 : 21) + pg_sym_any(r, c);
                neg = false;
            } else {
                if (!((i == bi && j == bj) || (i == bj && j == bi))) continue;
                off = 42 + (i == bi ? r * 6 + c : c * 6 + r);     // A_ij = -X, A_ji = -X^T
                neg = true;
            }
            for (int32_t ch = 0; ch < d.sp_chunks; ++ch) {
                const double v = d.sp_part[((size_t)p * d.sp_chunks + ch) * PG_SP + off];
                acc += neg ? -v : v;
            }
        }
        if (d.dn_chunks) {
            const int32_t o0 = bi == bj ? 0 : bj, o1 = bi == bj ? N : bj + 1;
            for (int32_t o = o0; o < o1; ++o) {
                if (o == bi) continue;
                const int32_t lo = o < bi ? o : bi, hi = o < bi ? bi : o;
                const int32_t slot = hi * (hi - 1) / 2 + lo;
                const int off = is_g ? 21 + r : pg_sym_any(r, c);
                // g: the target's entries lose h, the source's gain it; A: +S on the diagonal, -S off it
                const bool neg = is_g ? pg_dense_target(d.cnt, lo, hi) == bi : bi != bj;
                for (int32_t ch = 0; ch < d.dn_chunks; ++ch) {
                    const double v = d.dn_part[((size_t)slot * d.dn_chunks + ch) * PG_DN + off];
                    acc += neg ? -v : v;
                }
            }
        }
    }
    if (is_g) {
        g[6 * bi + r] = acc;
        if (dbg_g) dbg_g[6 * bi + r] = acc;
    } else {
        const size_t at = (size_t)(6 * bi + r) * n + 6 * bj + c;
        A[at] = acc;
        if (dbg_A) dbg_A[at] = acc;
    }
}

// Exp of delta = [omega, v] -> E[12] = rows of [R | t].
__device__ __forceinline__ void exp_se3(const double (&x)[6], double (&E)[12]) {
    const double wx = x[0], wy = x[1], wz = x[2], vx = x[3], vy = x[4], vz = x[5];
    const double th2 = (wx * wx + wy * wy) + wz * wz;
    const double cr[3] = {wy * vz - wz * vy, wz * vx - wx * vz, wx * vy - wy * vx};
    double A, B, t[3];
    if (th2 < 1e-8) {
        A = 1.0 - th2 / 6.0;
        B = 0.5;
        t[0] = vx + 0.5 * cr[0];
        t[1] = vy + 0.5 * cr[1];
        t[2] = vz + 0.5 * cr[2];
    } else {
        double C;
        if (th2 < 1e-6) {
            C = (1.0 - th2 / 20.0) / 6.0;
            A = 1.0 - th2 * C;
            B = 0.5 - th2 / 24.0;
        } else {
            const double th = sqrt(th2);
            A = sin(th) / th;
            B = (1.0 - cos(th)) / th2;
            C = (1.0 - A) / th2;
        }
        const double wc[3] = {wy * cr[2] - wz * cr[1], wz * cr[0] - wx * cr[2], wx * cr[1] - wy * cr[0]};
        t[0] = (vx + B * cr[0]) + C * wc[0];
        t[1] = (vy + B * cr[1]) + C * wc[1];
        t[2] = (vz + B * cr[2]) + C * wc[2];
    }
    E[0] = 1.0 - B * (wy * wy + wz * wz);
    E[1] = B * (wx * wy) - A * wz;
    E[2] = B * (wx * wz) + A * wy;
    E[3] = t[0];
    E[4] = B * (wx * wy) + A * wz;
    E[5] = 1.0 - B * (wx * wx + wz * wz);
    E[6] = B * (wy * wz) - A * wx;
    E[7] = t[1];
    E[8] = B * (wx * wz) - A * wy;
    E[9] = B * (wy * wz) + A * wx;
    E[10] = 1.0 - B * (wx * wx + wy * wy);
    E[11] = t[2];
}

// a . b over n <= PG_MAX_VARS entries of LDS, in the order of the header; every thread gets the sum.
__device__ __forceinline__ double pg_dot(const double *a, const double *b, int32_t n, double *red) {
    double acc = 0.0;
    for (int32_t r = threadIdx.x; r < n; r += 256) acc += a[r] * b[r];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    __syncthreads();                                             // the last sum has been read
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void k_pg_solve(int32_t N, int32_t n_inner, int32_t final_pass,
                                                  const double *__restrict__ A, const double *__restrict__ g,
                                                  const uint8_t *__restrict__ fixed, double *__restrict__ T,
                                                  const double *__restrict__ totals, double *__restrict__ history_row,
                                                  double *__restrict__ dbg_delta, double *__restrict__ iter_poses,
                                                  double *__restrict__ poses_out) {
    __shared__ double x[PG_MAX_VARS], rr[PG_MAX_VARS], z[PG_MAX_VARS], p[PG_MAX_VARS], Ap[PG_MAX_VARS], Mi[PG_MAX_VARS];
    __shared__ double red[4];
    const int32_t n = 6 * N;
    if (threadIdx.x < 4) history_row[threadIdx.x] = totals[threadIdx.x];
    if (final_pass) {
        for (int32_t k = threadIdx.x; k < N * 16; k += 256) poses_out[k] = T[k];
        return;
    }
    for (int32_t r = threadIdx.x; r < n; r += 256) {
        const double dgl = A[(size_t)r * n + r];
        Mi[r] = dgl > PG_EPS ? 1.0 / dgl : 1.0;
        x[r] = 0.0;
        rr[r] = g[r];
        z[r] = Mi[r] * rr[r];
        p[r] = z[r];
    }
    __syncthreads();
    double rz = pg_dot(rr, z, n, red);
    for (int32_t it = 0; it < n_inner; ++it) {
        for (int32_t r = threadIdx.x; r < n; r += 256) {
            double acc = 0.0;
            for (int32_t c = 0; c < n; ++c) acc += A[(size_t)c * n + r] * p[c];      // A is symmetric bit for bit: column r read as a row
            Ap[r] = acc;
        }
        __syncthreads();
        const double pAp = pg_dot(p, Ap, n, red);
        const double alpha = pAp > PG_EPS ? rz / pAp : 0.0;
        for (int32_t r = threadIdx.x; r < n; r += 256) {
            x[r] = x[r] + alpha * p[r];
            rr[r] = rr[r] - alpha * Ap[r];
            z[r] = Mi[r] * rr[r];
        }
        __syncthreads();
        const double rz_new = pg_dot(z, rr, n, red);
        const double beta = rz > PG_EPS ? rz_new / rz : 0.0;
        for (int32_t r = threadIdx.x; r < n; r += 256) p[r] = z[r] + beta * p[r];
        rz = rz_new;
        __syncthreads();
    }
    if (dbg_delta)
        for (int32_t r = threadIdx.x; r < n; r += 256) dbg_delta[r] = x[r];
    if ((int32_t)threadIdx.x < N) {
        const int32_t k = threadIdx.x;
        double Tk[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) Tk[e] = T[(size_t)k * 16 + e];
        if (!fixed[k]) {
            double dk[6], E[12], Tn[12];
#pragma unroll
            for (int e = 0; e < 6; ++e) dk[e] = x[6 * k + e];
            exp_se3(dk, E);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    double v = (E[r * 4] * Tk[c] + E[r * 4 + 1] * Tk[4 + c]) + E[r * 4 + 2] * Tk[8 + c];
                    if (c == 3) v = v + E[r * 4 + 3];
                    Tn[r * 4 + c] = v;
                }
#pragma unroll
            for (int e = 0; e < 12; ++e) Tk[e] = Tn[e];
#pragma unroll
            for (int e = 0; e < 12; ++e) T[(size_t)k * 16 + e] = Tk[e];
        }
        if (iter_poses) {
#pragma unroll
            for (int e = 0; e < 16; ++e) iter_poses[(size_t)k * 16 + e] = Tk[e];
        }
    }
}

// The workspace: T [N,16] f64 | cnt [N] i32 | sp_part [P, sp_chunks, 92] f64 | dn_part [N (N - 1) / 2,
// dn_chunks, 29] f64 | A [6N,6N] f64 | g [6N] f64 | totals [4] f64, each part aligned to 256 bytes. The
// size export reads `bytes` of a null base, the entry point the pointers into the caller's buffer.
struct PgPlan : Carver {
    int32_t sp_chunks, dn_chunks;
    double *T, *sp_part, *dn_part, *A, *g, *totals;
    int32_t *cnt;
    PgPlan(void *base, int32_t N, int32_t P, int64_t M, int32_t H, int32_t W) : Carver(base) {
        const uint64_t mean_tiles = P > 0 ? div_up((uint64_t)(M > 0 ? M : 0), (uint64_t)P * PG_TILE) : 0;
        sp_chunks = P > 0 ? (int32_t)(2 * mean_tiles < 1 ? 1 : (2 * mean_tiles > PG_SP_MAX_CHUNKS ? PG_SP_MAX_CHUNKS : 2 * mean_tiles)) : 0;
        const uint64_t tiles = (H > 0 && W > 0) ? div_up((uint64_t)H * (uint64_t)W, PG_TILE) : 0;
        dn_chunks = (int32_t)(tiles > PG_DN_MAX_CHUNKS ? PG_DN_MAX_CHUNKS : tiles);
        const size_t n = 6 * (size_t)N;
        T = take<double>((size_t)N * 16);
        cnt = take<int32_t>((size_t)N);
        sp_part = take<double>((size_t)P * sp_chunks * PG_SP);
        dn_part = take<double>((size_t)N * (N - 1) / 2 * dn_chunks * PG_DN);
        A = take<double>(n * n);
        g = take<double>(n);
        totals = take<double>(4);
    }
};

}  // namespace nof

using namespace nof;

extern "C" {

size_t nof_pose_graph_workspace_bytes(int32_t N, int32_t P, int64_t M, int32_t H, int32_t W) {
    if (N < 1 || N > PG_MAX_FRAMES || P < 0 || M < 0 || H < 0 || W < 0 || (int64_t)H * W >= (1ll << 24)) return 0;
    return PgPlan(nullptr, N, P, M, H, W).bytes;
}

int nof_pose_graph_optimize(const nof_pose_graph_desc *d, void *stream) {
    const char *fn = "pose_graph_optimize";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (d->N < 1 || d->N > PG_MAX_FRAMES) return set_error(NOF_EINVAL, "%s: N=%d must be in 1..%d", fn, d->N, PG_MAX_FRAMES);
    if (d->n_outer < 1 || d->n_outer > 1024) return set_error(NOF_EINVAL, "%s: n_outer=%d must be in 1..1024", fn, d->n_outer);
    if (d->n_inner < 0 || d->n_inner > 1024) return set_error(NOF_EINVAL, "%s: n_inner=%d must be in 0..1024", fn, d->n_inner);
    if (d->P < 0 || d->P > 65535) return set_error(NOF_EINVAL, "%s: P=%d must be in 0..65535", fn, d->P);
    if (d->M < 0 || d->M >= (1ll << 31)) return set_error(NOF_EINVAL, "%s: M=%lld must be in 0..2^31-1", fn, (long long)d->M);
    const bool sparse = d->P > 0, dense = d->points != nullptr || d->normals != nullptr;
    if (!sparse && !dense) return set_error(NOF_EINVAL, "%s: neither pair_frames (P=0) nor points is given", fn);
    if (!(d->robust_delta > 0)) return set_error(NOF_EINVAL, "%s: robust_delta=%g must be positive", fn, d->robust_delta);
    if (sparse) {
        if (!(d->w_sparse >= 0)) return set_error(NOF_EINVAL, "%s: w_sparse=%g must not be negative", fn, d->w_sparse);
        if (int rc = require_pointers(fn, {{d->pair_frames, "pair_frames"}, {d->pair_start, "pair_start"},
                                           {d->pts_a, "pts_a", d->M > 0}, {d->pts_b, "pts_b", d->M > 0}}))
            return rc;
    }
    if (dense) {
        if (!d->points || !d->normals)
            return set_error(NOF_EINVAL, "%s: %s is NULL while the other map is given", fn, d->points ? "normals" : "points");
        if (d->H < 1 || d->W < 1 || (int64_t)d->H * d->W >= (1ll << 24))
            return set_error(NOF_EINVAL, "%s: H=%d W=%d must be positive with H W < 2^24", fn, d->H, d->W);
        if (d->radius < 0 || d->radius > PG_MAX_RADIUS)
            return set_error(NOF_EINVAL, "%s: radius=%d must be in 0..%d", fn, d->radius, PG_MAX_RADIUS);
        if (!(d->dist_thresh > 0)) return set_error(NOF_EINVAL, "%s: dist_thresh=%g must be positive", fn, d->dist_thresh);
        if (!(d->w_dense >= 0)) return set_error(NOF_EINVAL, "%s: w_dense=%g must not be negative", fn, d->w_dense);
        if (d->normal_thresh != d->normal_thresh || d->min_trace != d->min_trace || d->depth_min != d->depth_min ||
            d->depth_max != d->depth_max)
            return set_error(NOF_EINVAL, "%s: normal_thresh, min_trace, depth_min or depth_max is NaN", fn);
        if (!(d->fx == d->fx && d->fy == d->fy && d->cx == d->cx && d->cy == d->cy))
            return set_error(NOF_EINVAL, "%s: fx, fy, cx or cy is NaN", fn);
    }
    if (int rc = require_pointers(fn, {{d->poses, "poses"}, {d->fixed, "fixed"}, {d->poses_out, "poses_out"},
                                       {d->history, "history"}, {d->workspace, "workspace"}}))
        return rc;
    const int32_t N = d->N, n = 6 * N, P = d->P, H = dense ? d->H : 0, W = dense ? d->W : 0;
    const PgPlan pl(d->workspace, N, P, d->M, H, W);
    if (int rc = require_workspace(fn, d->workspace_bytes, pl.bytes)) return rc;

    hipStream_t s = (hipStream_t)stream;
    double *T = pl.T, *sp_part = pl.sp_part, *dn_part = pl.dn_part, *A = pl.A, *g = pl.g, *totals = pl.totals;
    int32_t *cnt = pl.cnt;
    const int32_t HW = H * W;
    PgDense dd;
    dd.points = d->points, dd.normals = d->normals;
    dd.N = N, dd.H = H, dd.W = W, dd.radius = d->radius;
    dd.fx = d->fx, dd.fy = d->fy, dd.cx = d->cx, dd.cy = d->cy;
    dd.delta = d->robust_delta, dd.w_dense = d->w_dense, dd.dist_thresh = d->dist_thresh;
    dd.normal_thresh = d->normal_thresh, dd.depth_min = d->depth_min, dd.depth_max = d->depth_max, dd.min_trace = d->min_trace;
    PgAssemble da;
    da.pair_frames = d->pair_frames, da.fixed = d->fixed, da.cnt = cnt, da.sp_part = sp_part, da.dn_part = dn_part;
    da.N = N, da.P = P, da.sp_chunks = pl.sp_chunks, da.dn_chunks = dense ? pl.dn_chunks : 0;

    hipLaunchKernelGGL(k_pg_prepare, dim3((unsigned)N), dim3(256), 0, s, d->poses, N, d->points, d->normals, HW,
                       d->depth_min, d->depth_max, T, cnt, d->iter_poses);
    for (int32_t k = 0; k <= d->n_outer; ++k) {
        const bool last = k == d->n_outer;                       // the energies at the final poses, no step
        if (sparse)
            hipLaunchKernelGGL(k_pg_sparse, dim3((unsigned)pl.sp_chunks, (unsigned)P), dim3(256), 0, s, d->pair_frames,
                               d->pts_a, d->pts_b, d->pair_start, d->weight, d->M, N, T, d->robust_delta, d->w_sparse,
                               sp_part);
        if (dense && N > 1)
            hipLaunchKernelGGL(k_pg_dense, dim3((unsigned)pl.dn_chunks, (unsigned)N, (unsigned)N), dim3(256), 0, s, dd, T,
                               cnt, dn_part,
                               (!last && d->dense_index) ? d->dense_index + (size_t)k * N * N * HW : nullptr);
        hipLaunchKernelGGL(k_pg_assemble, dim3(last ? 1u : (unsigned)(N * N + 1)), dim3(256), 0, s, da, last ? 1 : 0, A, g,
                           totals, (!last && d->dbg_A) ? d->dbg_A + (size_t)k * n * n : nullptr,
                           (!last && d->dbg_g) ? d->dbg_g + (size_t)k * n : nullptr);
        hipLaunchKernelGGL(k_pg_solve, dim3(1), dim3(256), 0, s, N, d->n_inner, last ? 1 : 0, A, g, d->fixed, T, totals,
                           d->history + (size_t)k * 4, (!last && d->dbg_delta) ? d->dbg_delta + (size_t)k * n : nullptr,
                           (!last && d->iter_poses) ? d->iter_poses + (size_t)(k + 1) * N * 16 : nullptr, d->poses_out);
    }
    return check_launch(fn);
}

}  // extern "C"
