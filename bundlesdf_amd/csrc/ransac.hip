// Multi-pair RANSAC over 3-D correspondences (include/nof.h group 8): which matches
// between two frames agree with one rigid motion. The reference's
// BundleTrack/src/cuda/cuda_ransac.cu keeps a [trials x points] flag array per pair,
// scores with float atomics and lets the last trial that equals the maximum win;
// here a trial's score is an int64 sum, the winner is the lowest trial of the
// highest score and the flags are recomputed from the winning pose alone.
//
//  k_ransac_hypotheses  one lane per (pair, trial): the three draws, Horn's
//                       quaternion fit of them (4x4 cyclic Jacobi), the gates; pose,
//                       live flag and a zeroed score go to the workspace.
//  k_ransac_score       the hot path, P T n row tests. A lane holds one trial's pose
//                       in registers; a block of 256 trials stages a tile of
//                       RANSAC_TILE rows in LDS once, one record per row, and all
//                       lanes walk the tile together: every LDS read is one address
//                       for the whole wave (a broadcast, no bank conflict) and a row
//                       leaves global memory once per 256 trials. blockIdx.z takes
//                       every gridDim.z-th tile of the pair, and the partial scores
//                       meet in one 64-bit integer atomicAdd per (trial, chunk).
//  k_ransac_best        one block per pair: argmax on (score descending, trial
//                       ascending), the winning pose or the identity.
//  k_ransac_flags       one block per pair: the rows against the winning pose, the
//                       flags, their count, min_inliers, and the 17 sums in a fixed
//                       thread -> row assignment and a fixed order of additions.
#include "geom_device.h"
#include "host_entry.h"

#pragma clang fp contract(off)

namespace nof {

constexpr int RANSAC_TILE = 256;      // rows staged per tile = threads of a block: one row per thread
constexpr int RANSAC_MAX_CHUNKS = 64;

__device__ __forceinline__ uint32_t ransac_hash(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// One Jacobi rotation of the symmetric 4x4 A in the (P, Q) plane, accumulated into V (Rutishauser's
// form: the update of each element is a small correction added to it).
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&A)[4][4], double (&V)[4][4], int sweep) {
    const double apq = A[P][Q];
    const double g = 100.0 * fabs(apq);
    if (sweep > 3 && fabs(A[P][P]) + g == fabs(A[P][P]) && fabs(A[Q][Q]) + g == fabs(A[Q][Q])) {
        A[P][Q] = A[Q][P] = 0.0;
        return;
    }
    if (!(fabs(apq) > 0.0)) return;
    const double h = A[Q][Q] - A[P][P];
    double t;
    if (fabs(h) + g == fabs(h)) {
        t = apq / h;
    } else {
        const double theta = 0.5 * h / apq;
        t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
    }
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double x = A[r][P], y = A[r][Q];
            A[r][P] = A[P][r] = x - s * (y + x * tau);
            A[r][Q] = A[Q][r] = y + s * (x - y * tau);
        }
        const double x = V[r][P], y = V[r][Q];
        V[r][P] = x - s * (y + x * tau);
        V[r][Q] = y + s * (x - y * tau);
    }
}

// Least-squares rigid fit b ~ R a + t of three pairs -> T[12] = rows of [R | t]. Horn 1987: the unit
// quaternion is the eigenvector of the largest eigenvalue of N(S), S = sum (a - mean a)(b - mean b)^T.
// R comes from the normalised quaternion, so it is a rotation of determinant +1 whatever the sample:
// for three pairs S has rank <= 2 and an SVD's third singular vectors would carry the reflection fix.
__device__ void rigid_fit3(const double (&a)[3][3], const double (&b)[3][3], double (&T)[12]) {
    double am[3], bm[3], S[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        am[k] = ((a[0][k] + a[1][k]) + a[2][k]) / 3.0;
        bm[k] = ((b[0][k] + b[1][k]) + b[2][k]) / 3.0;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            S[r][c] = ((a[0][r] - am[r]) * (b[0][c] - bm[c]) + (a[1][r] - am[r]) * (b[1][c] - bm[c])) +
                      (a[2][r] - am[r]) * (b[2][c] - bm[c]);
    double A[4][4], V[4][4];
    A[0][0] = (S[0][0] + S[1][1]) + S[2][2];
    A[1][1] = (S[0][0] - S[1][1]) - S[2][2];
    A[2][2] = (S[1][1] - S[0][0]) - S[2][2];
    A[3][3] = (S[2][2] - S[0][0]) - S[1][1];
    A[0][1] = A[1][0] = S[1][2] - S[2][1];
    A[0][2] = A[2][0] = S[2][0] - S[0][2];
    A[0][3] = A[3][0] = S[0][1] - S[1][0];
    A[1][2] = A[2][1] = S[0][1] + S[1][0];
    A[1][3] = A[3][1] = S[2][0] + S[0][2];
    A[2][3] = A[3][2] = S[1][2] + S[2][1];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 16; ++sweep) {
        const double off = ((fabs(A[0][1]) + fabs(A[0][2])) + (fabs(A[0][3]) + fabs(A[1][2]))) +
                           (fabs(A[1][3]) + fabs(A[2][3]));
        if (off == 0.0) break;      // NaN runs the sweeps out and ends as a dead trial
        jacobi_rotate<0, 1>(A, V, sweep);
        jacobi_rotate<0, 2>(A, V, sweep);
        jacobi_rotate<0, 3>(A, V, sweep);
        jacobi_rotate<1, 2>(A, V, sweep);
        jacobi_rotate<1, 3>(A, V, sweep);
        jacobi_rotate<2, 3>(A, V, sweep);
    }
    double best = A[0][0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        if (A[k][k] > best) {
            best = A[k][k];
#pragma unroll
            for (int r = 0; r < 4; ++r) q[r] = V[r][k];
        }
    }
    const double len = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    const double w = q[0] / len, x = q[1] / len, y = q[2] / len, z = q[3] / len;
    double R[3][3];
    R[0][0] = 1.0 - 2.0 * (y * y + z * z);
    R[1][1] = 1.0 - 2.0 * (x * x + z * z);
    R[2][2] = 1.0 - 2.0 * (x * x + y * y);
    R[0][1] = 2.0 * (x * y - w * z);
    R[1][0] = 2.0 * (x * y + w * z);
    R[0][2] = 2.0 * (x * z + w * y);
    R[2][0] = 2.0 * (x * z - w * y);
    R[1][2] = 2.0 * (y * z - w * x);
    R[2][1] = 2.0 * (y * z + w * x);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        T[k * 4] = R[k][0];
        T[k * 4 + 1] = R[k][1];
        T[k * 4 + 2] = R[k][2];
        T[k * 4 + 3] = bm[k] - ((R[k][0] * am[0] + R[k][1] * am[1]) + R[k][2] * am[2]);
    }
}

struct RansacWs {
    double *pose;       // [P,T,12]
    int64_t *score;     // [P,T]
    uint8_t *live;      // [P,T]
};

__global__ __launch_bounds__(256) void k_ransac_hypotheses(const double *__restrict__ pts_a,
                                                           const double *__restrict__ pts_b,
                                                           const int32_t *__restrict__ pair_start, int64_t M, int32_t T,
                                                           uint32_t seed_hash, const double *__restrict__ max_trans_sq,
                                                           const double *__restrict__ min_trace, RansacWs ws,
                                                           int32_t *__restrict__ trial_idx,
                                                           double *__restrict__ trial_pose,
                                                           uint8_t *__restrict__ trial_live) {
    const int32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int32_t p = blockIdx.y;
    int64_t s;
    int32_t n;
    pair_rows(pair_start, p, M, s, n);
    const size_t pt = (size_t)p * T + t;
    const uint32_t counter = ((uint32_t)p * (uint32_t)T + (uint32_t)t) * 3u;
    int32_t idx[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) idx[j] = (int32_t)(((uint64_t)ransac_hash((counter + j) ^ seed_hash) * (uint64_t)n) >> 32);
    bool live = n >= 3 && idx[0] != idx[1] && idx[0] != idx[2] && idx[1] != idx[2];
    double pose[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = 0.0;
    if (live) {
        double a[3][3], b[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                a[j][k] = pts_a[(size_t)(s + idx[j]) * 3 + k];     // idx < n: inside the pair, inside [0, M)
                b[j][k] = pts_b[(size_t)(s + idx[j]) * 3 + k];
            }
        rigid_fit3(a, b, pose);
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 12; ++k) finite = finite && fabs(pose[k]) <= 1.7976931348623157e308;    // false for NaN
        const double t2 = (pose[3] * pose[3] + pose[7] * pose[7]) + pose[11] * pose[11];
        const double tr = (pose[0] + pose[5]) + pose[10];
        live = finite && t2 <= max_trans_sq[p] && tr >= min_trace[p];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) ws.pose[pt * 12 + k] = pose[k];
    ws.live[pt] = live ? 1 : 0;
    ws.score[pt] = 0;
    if (trial_idx) {
#pragma unroll
        for (int j = 0; j < 3; ++j) trial_idx[pt * 3 + j] = idx[j];
    }
    if (trial_pose) {
#pragma unroll
        for (int k = 0; k < 12; ++k) trial_pose[pt * 12 + k] = pose[k];
    }
    if (trial_live) trial_live[pt] = live ? 1 : 0;
}

// One staged row: everything the inlier test reads, side by side, so that the walk fetches it with
// 16-byte LDS reads from one address per wave.
template <bool NORMALS> struct RansacRow;
template <> struct alignas(16) RansacRow<false> {
    double a[3], b[3];
    int64_t w;
    double pad;
};
template <> struct alignas(16) RansacRow<true> {
    double a[3], b[3], na[3], nb[3];
    int64_t w;
    double pad;
};

// The inlier test of include/nof.h, one row against one pose (rows of [R | t]).
template <bool NORMALS>
__device__ __forceinline__ bool ransac_inlier(const double (&T)[12], const RansacRow<NORMALS> &r, double dist_sq,
                                              double cos_normal) {
    double a[3];
    xform_point(T, r.a[0], r.a[1], r.a[2], a);
    const double dx = r.b[0] - a[0], dy = r.b[1] - a[1], dz = r.b[2] - a[2];
    bool in = (dx * dx + dy * dy) + dz * dz <= dist_sq;
    if constexpr (NORMALS) {
        double n[3];
        xform_dir(T, r.na[0], r.na[1], r.na[2], n);
        in = in && (n[0] * r.nb[0] + n[1] * r.nb[1]) + n[2] * r.nb[2] >= cos_normal;
    }
    return in;
}

template <bool NORMALS>
__device__ __forceinline__ void ransac_load_row(RansacRow<NORMALS> &r, int64_t i, const double *__restrict__ pts_a,
                                                const double *__restrict__ pts_b, const double *__restrict__ normals_a,
                                                const double *__restrict__ normals_b, const double *__restrict__ conf) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.a[k] = pts_a[(size_t)i * 3 + k];
        r.b[k] = pts_b[(size_t)i * 3 + k];
        if constexpr (NORMALS) {
            r.na[k] = normals_a[(size_t)i * 3 + k];
            r.nb[k] = normals_b[(size_t)i * 3 + k];
        }
    }
    r.w = conf ? __double2ll_rn(conf[i] * 65536.0) : 65536ll;
}

template <bool NORMALS>
__global__ __launch_bounds__(256) void k_ransac_score(const double *__restrict__ pts_a, const double *__restrict__ pts_b,
                                                      const double *__restrict__ normals_a,
                                                      const double *__restrict__ normals_b,
                                                      const double *__restrict__ conf,
                                                      const int32_t *__restrict__ pair_start, int64_t M, int32_t T,
                                                      double dist_sq, double cos_normal, RansacWs ws) {
    __shared__ RansacRow<NORMALS> rows[RANSAC_TILE];
    const int32_t p = blockIdx.y;
    int64_t s;
    int32_t n;
    pair_rows(pair_start, p, M, s, n);
    const int32_t n_tiles = (n + RANSAC_TILE - 1) / RANSAC_TILE;
    if ((int32_t)blockIdx.z >= n_tiles) return;               // the whole block leaves
    const int32_t t = blockIdx.x * 256 + threadIdx.x;
    const size_t pt = (size_t)p * T + (t < T ? t : 0);
    const bool live = t < T && ws.live[pt] != 0;
    if (!__syncthreads_or(live)) return;                      // 256 dead trials: no walk
    double pose[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = live ? ws.pose[pt * 12 + k] : 0.0;
    int64_t acc = 0;
    for (int32_t tile = blockIdx.z; tile < n_tiles; tile += gridDim.z) {
        const int32_t r0 = tile * RANSAC_TILE;
        const int32_t cnt = n - r0 < RANSAC_TILE ? n - r0 : RANSAC_TILE;
        __syncthreads();                                      // the previous tile has been walked
        if ((int32_t)threadIdx.x < cnt)
            ransac_load_row<NORMALS>(rows[threadIdx.x], s + r0 + threadIdx.x, pts_a, pts_b, normals_a, normals_b, conf);
        __syncthreads();
        if (live) {
#pragma unroll 4
            for (int32_t r = 0; r < cnt; ++r) {
                const RansacRow<NORMALS> row = rows[r];
                acc += ransac_inlier<NORMALS>(pose, row, dist_sq, cos_normal) ? row.w : 0ll;
            }
        }
    }
    if (live && acc != 0) atomicAdd((unsigned long long *)&ws.score[pt], (unsigned long long)acc);
}

__global__ __launch_bounds__(256) void k_ransac_best(int32_t T, RansacWs ws, int32_t *__restrict__ best_trial,
                                                     int64_t *__restrict__ score, double *__restrict__ pose,
                                                     int64_t *__restrict__ trial_score) {
    __shared__ int64_t wave_score[4];
    __shared__ int32_t wave_trial[4];
    const int32_t p = blockIdx.x;
    const size_t base = (size_t)p * T;
    int64_t bs = 0;
    int32_t bt = -1;
    for (int32_t t = threadIdx.x; t < T; t += 256) {          // ascending t: a later equal score does not win
        const int64_t sc = ws.live[base + t] ? ws.score[base + t] : 0;
        if (trial_score) trial_score[base + t] = sc;
        if (sc > bs) {
            bs = sc;
            bt = t;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int64_t os = __shfl_xor(bs, o, 64);
        const int32_t ot = __shfl_xor(bt, o, 64);
        if (os > bs || (os == bs && os > 0 && ot < bt)) {
            bs = os;
            bt = ot;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        wave_score[threadIdx.x >> 6] = bs;
        wave_trial[threadIdx.x >> 6] = bt;
    }
    __syncthreads();
    bs = wave_score[0];
    bt = wave_trial[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        if (wave_score[w] > bs || (wave_score[w] == bs && bs > 0 && wave_trial[w] < bt)) {
            bs = wave_score[w];
            bt = wave_trial[w];
        }
    }
    if (threadIdx.x == 0) {
        best_trial[p] = bt;
        score[p] = bs;
    }
    if (threadIdx.x < 16) {
        const int k = threadIdx.x;
        double v = (k % 5 == 0) ? 1.0 : 0.0;
        if (bt >= 0 && k < 12) v = ws.pose[(base + bt) * 12 + k];
        pose[(size_t)p * 16 + k] = v;
    }
}

template <bool NORMALS>
__global__ __launch_bounds__(256) void k_ransac_flags(const double *__restrict__ pts_a, const double *__restrict__ pts_b,
                                                      const double *__restrict__ normals_a,
                                                      const double *__restrict__ normals_b,
                                                      const int32_t *__restrict__ pair_start, int64_t M,
                                                      double dist_sq, double cos_normal, int32_t min_inliers,
                                                      const int32_t *__restrict__ best_trial,
                                                      const double *__restrict__ pose_out,
                                                      uint8_t *__restrict__ inlier, int32_t *__restrict__ n_inliers,
                                                      double *__restrict__ sums) {
    __shared__ double wave_sum[4][RIGID_SUMS];
    const int32_t p = blockIdx.x;
    int64_t s;
    int32_t n;
    pair_rows(pair_start, p, M, s, n);
    const bool won = best_trial[p] >= 0;
    double pose[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = pose_out[(size_t)p * 16 + k];
    double acc[RIGID_SUMS];
#pragma unroll
    for (int k = 0; k < RIGID_SUMS; ++k) acc[k] = 0.0;
    for (int32_t r = threadIdx.x; r < n; r += 256) {
        const int64_t i = s + r;
        RansacRow<NORMALS> row;
        ransac_load_row<NORMALS>(row, i, pts_a, pts_b, normals_a, normals_b, nullptr);
        const bool in = won && ransac_inlier<NORMALS>(pose, row, dist_sq, cos_normal);
        inlier[i] = in ? 1 : 0;
        if (in) {
            rigid_moments_add(acc, row.a, row.b);
            const double dx = row.b[0] - row.a[0], dy = row.b[1] - row.a[1], dz = row.b[2] - row.a[2];
            acc[16] += (dx * dx + dy * dy) + dz * dz;
        }
    }
    block_sum_waves<RIGID_SUMS>(acc, wave_sum);
    // the count is a sum of ones below 2^31: exact in f64
    const double count = wave_total<RIGID_SUMS>(wave_sum, 0);
    const bool clear = count < (double)min_inliers;
    if (threadIdx.x < RIGID_SUMS)
        sums[(size_t)p * RIGID_SUMS + threadIdx.x] = clear ? 0.0 : wave_total<RIGID_SUMS>(wave_sum, threadIdx.x);
    if (threadIdx.x == 0) n_inliers[p] = clear ? 0 : (int32_t)count;
    if (clear) {
        for (int32_t r = threadIdx.x; r < n; r += 256) inlier[s + r] = 0;     // each thread rewrites its own rows
    }
}

// One part: the three arrays lie packed in it, and only their sum is rounded up.
struct RansacPlan : Carver {
    RansacWs ws{};
    RansacPlan(void *base, int32_t P, int32_t T) : Carver(base) {
        const size_t pt = (size_t)P * (size_t)T;
        ws.pose = (double *)take<char>(pt * (12 * sizeof(double) + sizeof(int64_t) + 1));
        if (!base) return;
        ws.score = (int64_t *)(ws.pose + pt * 12);
        ws.live = (uint8_t *)(ws.score + pt);
    }
};

}  // namespace nof

using namespace nof;

extern "C" {

size_t nof_ransac_workspace_bytes(int32_t P, int64_t M, int32_t n_trials) {
    (void)M;    // nothing is kept per row
    if (P < 1 || n_trials < 1) return 0;
    return RansacPlan(nullptr, P, n_trials).bytes;
}

int nof_ransac_pairs(const nof_ransac_desc *d, void *stream) {
    const char *fn = "ransac_pairs";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (d->P < 1 || d->P > 65535) return set_error(NOF_EINVAL, "%s: P=%d must be in 1..65535", fn, d->P);
    if (d->n_trials < 1 || d->n_trials > 65536)
        return set_error(NOF_EINVAL, "%s: n_trials=%d must be in 1..65536", fn, d->n_trials);
    if (d->M < 0 || d->M >= (1ll << 31))
        return set_error(NOF_EINVAL, "%s: M=%lld must be in 0..2^31-1", fn, (long long)d->M);
    if ((d->normals_a == nullptr) != (d->normals_b == nullptr))
        return set_error(NOF_EINVAL, "%s: %s is NULL while the other side's normals are given", fn,
                         d->normals_a ? "normals_b" : "normals_a");
    if (!(d->inlier_dist_sq >= 0))
        return set_error(NOF_EINVAL, "%s: inlier_dist_sq=%g must not be negative", fn, d->inlier_dist_sq);
    if (d->normals_a && d->cos_normal != d->cos_normal) return set_error(NOF_EINVAL, "%s: cos_normal is NaN", fn);
    const bool rows = d->M > 0;
    if (int rc = require_pointers(fn, {{d->best_trial, "best_trial"}, {d->score, "score"}, {d->pose, "pose"},
                                       {d->n_inliers, "n_inliers"}, {d->sums, "sums"}, {d->inlier, "inlier", rows},
                                       {d->pts_a, "pts_a", rows}, {d->pts_b, "pts_b", rows},
                                       {d->pair_start, "pair_start", rows}, {d->max_trans_sq, "max_trans_sq", rows},
                                       {d->min_trace, "min_trace", rows}, {d->workspace, "workspace", rows}}))
        return rc;
    if (d->M == 0) return NOF_OK;
    const int32_t P = d->P, T = d->n_trials;
    const RansacPlan pl(d->workspace, P, T);
    if (int rc = require_workspace(fn, d->workspace_bytes, pl.bytes)) return rc;

    hipStream_t s = (hipStream_t)stream;
    const RansacWs ws = pl.ws;
    uint32_t seed_hash = d->seed;                            // ransac_hash on the host
    seed_hash ^= seed_hash >> 16;
    seed_hash *= 0x7feb352du;
    seed_hash ^= seed_hash >> 15;
    seed_hash *= 0x846ca68bu;
    seed_hash ^= seed_hash >> 16;
    const dim3 trials(div_up(T, 256), (unsigned)P);
    hipLaunchKernelGGL(k_ransac_hypotheses, trials, dim3(256), 0, s, d->pts_a, d->pts_b, d->pair_start, d->M, T,
                       seed_hash, d->max_trans_sq, d->min_trace, ws, d->trial_idx, d->trial_pose, d->trial_live);
    // row chunks: four times the mean tile count of a pair, so that an uneven call still spreads its
    // long pairs; a chunk beyond a pair's last tile leaves at once
    const uint64_t mean_tiles = div_up((uint64_t)d->M, (uint64_t)P * RANSAC_TILE);
    const unsigned chunks = (unsigned)(4 * mean_tiles < (uint64_t)RANSAC_MAX_CHUNKS ? 4 * mean_tiles : RANSAC_MAX_CHUNKS);
    const dim3 grid(trials.x, (unsigned)P, chunks);
    if (d->normals_a) {
        hipLaunchKernelGGL(k_ransac_score<true>, grid, dim3(256), 0, s, d->pts_a, d->pts_b, d->normals_a, d->normals_b,
                           d->conf, d->pair_start, d->M, T, d->inlier_dist_sq, d->cos_normal, ws);
    } else {
        hipLaunchKernelGGL(k_ransac_score<false>, grid, dim3(256), 0, s, d->pts_a, d->pts_b, d->normals_a, d->normals_b,
                           d->conf, d->pair_start, d->M, T, d->inlier_dist_sq, d->cos_normal, ws);
    }
    hipLaunchKernelGGL(k_ransac_best, dim3((unsigned)P), dim3(256), 0, s, T, ws, d->best_trial, d->score, d->pose,
                       d->trial_score);
    if (d->normals_a) {
        hipLaunchKernelGGL(k_ransac_flags<true>, dim3((unsigned)P), dim3(256), 0, s, d->pts_a, d->pts_b, d->normals_a,
                           d->normals_b, d->pair_start, d->M, d->inlier_dist_sq, d->cos_normal, d->min_inliers,
                           d->best_trial, d->pose, d->inlier, d->n_inliers, d->sums);
    } else {
        hipLaunchKernelGGL(k_ransac_flags<false>, dim3((unsigned)P), dim3(256), 0, s, d->pts_a, d->pts_b, d->normals_a,
                           d->normals_b, d->pair_start, d->M, d->inlier_dist_sq, d->cos_normal, d->min_inliers,
                           d->best_trial, d->pose, d->inlier, d->n_inliers, d->sums);
    }
    return check_launch(fn);
}

}  // extern "C"
