// Pair crops (include/nof.h group 15): each frame's mask bounding box, and the masked, rotated, scaled
// square crops the matcher is shown instead of whole frames. The reference's Frame::updateRoi
// (BundleTrack/src/Frame.cpp) and the two cv::warpPerspective calls at the end of processImagePair
// (BundleTrack/src/FeatureManager.cpp) over images that Frame::invalidatePixel has zeroed outside the mask.
// The transforms themselves are formed on the host (bundlesdf_amd/pairs.py); the kernel receives their
// inverses.
//
// This comment is the definition; tests/pair_crop_oracle.py restates it in numpy float64. Pixel (u, v) =
// (column, row), images row-major. All floating-point arithmetic is IEEE float64 in the order written
// here, without contraction; an output is rounded once to float32. No floating-point atomics and no
// floating-point reductions: the same bytes on every run.
//
//  k_mask_roi   masks [N,H,W] u8 -> roi [N,4] i32 = (umin, umax, vmin, vmax), inclusive, over the pixels
//               with mask > 0, and count [N] i32 = the number of such pixels. The call first writes
//               roi = (W, -1, H, -1) and count = 0 (k_mask_roi_init), which is what an empty mask keeps.
//               Integers only: a block reduces its 64 x 32 pixels by wave shuffles and LDS, then a
//               block that saw a pixel issues atomicMin / atomicMax / atomicAdd on its frame's entries.
//  k_pair_warp  Q crops of side S, out [Q,S,S] f32. Crop q reads frame f = frames[q] through m = inv[q],
//               a [2,3] f64 row-major affine map from crop pixel to source pixel. f outside 0 .. N-1:
//               the crop and its cells are zeros and nothing is read. Source value val(u, v):
//                 u8 grey:  (double)g / 255.0
//                 f32 grey: (double)g
//                 u8 RGB:   ((0.2989 (double)R + 0.587 (double)G) + 0.114 (double)B) / 255.0
//               v(u, v) = 0.0 if (u, v) lies outside the image or a mask is given and mask[f,v,u] == 0,
//               else val(u, v). For the output pixel (x, y), x and y integers converted exactly:
//                 sx = (m00 x + m01 y) + m02;   sy = (m10 x + m11 y) + m12
//                 unless sx >= -1 and sx < W and sy >= -1 and sy < H (NaN fails): out = 0, no tap read
//                 x0 = floor(sx), fx = sx - x0;   y0 = floor(sy), fy = sy - y0
//                 top = v(x0, y0) (1 - fx) + v(x0+1, y0) fx;   bot = v(x0, y0+1) (1 - fx) + v(x0+1, y0+1) fx
//                 out = f32(top (1 - fy) + bot fy)
//               (every tap of a pixel that fails the range test is outside the image, so that test only
//               keeps floor away from values an int cannot hold). Cells [Q, S/8, S/8] u8, optional:
//               cell (cx, cy) = 1 iff one of its 64 crop pixels has nu = floor(sx + 0.5), nv =
//               floor(sy + 0.5) with 0 <= sx + 0.5 < W and 0 <= sy + 0.5 < H (compared as doubles) and,
//               when a mask is given, mask[f, nv, nu] != 0.
//
// Shape. k_pair_warp: one thread per crop pixel, a block of 256 owns 32 columns x 8 rows of one crop (four
// cells side by side), a wave two rows of 32; the 32 float32 of a row are one 128-byte store, and a wave's
// taps fall on a few source rows and go through the vector cache (a gather; nothing is staged in LDS). Each
// wave ballots its nearest-pixel flags, lane 0 leaves the 64 bits in LDS, and threads 0 .. 3 form the
// block's four cell bytes. Blocks are numbered crop-major along x, so Q has no grid limit of its own.
#include "host_entry.h"

#pragma clang fp contract(off)

namespace nof {

constexpr int PC_BX = 32, PC_BY = 8;              // k_pair_warp: a block's crop pixels, one per thread
constexpr int ROI_BX = 64, ROI_BY = 4;            // k_mask_roi: threads of a block
constexpr int ROI_ROWS = 32;                      // rows of pixels a block takes, ROI_ROWS / ROI_BY per thread
constexpr int PC_MAX_SIDE = 4096;

__global__ void k_mask_roi_init(int32_t *__restrict__ roi, int32_t *__restrict__ count, int N, int H, int W) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= N) return;
    roi[f * 4] = W, roi[f * 4 + 1] = -1, roi[f * 4 + 2] = H, roi[f * 4 + 3] = -1;
    count[f] = 0;
}

__device__ __forceinline__ int roi_wave_min(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ int roi_wave_max(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ int roi_wave_sum(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__global__ __launch_bounds__(256) void k_mask_roi(const uint8_t *__restrict__ masks, int H, int W,
                                                  int32_t *__restrict__ roi, int32_t *__restrict__ count) {
    __shared__ int32_t part[ROI_BY][5];
    const int f = blockIdx.z;
    const uint8_t *m = masks + (size_t)f * H * W;
    const int u = blockIdx.x * ROI_BX + threadIdx.x;
    int umin = W, umax = -1, vmin = H, vmax = -1, n = 0;
    if (u < W) {
        for (int r = threadIdx.y; r < ROI_ROWS; r += ROI_BY) {
            const int v = blockIdx.y * ROI_ROWS + r;
            if (v < H && m[(size_t)v * W + u] > 0) {
                umin = min(umin, u), umax = max(umax, u), vmin = min(vmin, v), vmax = max(vmax, v);
                n += 1;
            }
        }
    }
    // threadIdx.y is the wave: every lane of every wave arrives here
    umin = roi_wave_min(umin), umax = roi_wave_max(umax), vmin = roi_wave_min(vmin), vmax = roi_wave_max(vmax);
    n = roi_wave_sum(n);
    if (threadIdx.x == 0) {
        int32_t *p = part[threadIdx.y];
        p[0] = umin, p[1] = umax, p[2] = vmin, p[3] = vmax, p[4] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        for (int w = 1; w < ROI_BY; ++w) {
            umin = min(umin, part[w][0]), umax = max(umax, part[w][1]);
            vmin = min(vmin, part[w][2]), vmax = max(vmax, part[w][3]);
            n += part[w][4];
        }
        if (n > 0) {
            atomicMin(&roi[f * 4], umin);
            atomicMax(&roi[f * 4 + 1], umax);
            atomicMin(&roi[f * 4 + 2], vmin);
            atomicMax(&roi[f * 4 + 3], vmax);
            atomicAdd(&count[f], n);
        }
    }
}

// The source forms of k_pair_warp: val(u, v) of the header comment at pixel index pix of the source array.
struct PcGreyU8 {
    static __device__ __forceinline__ double val(const void *__restrict__ src, size_t pix) {
        return (double)static_cast<const uint8_t *>(src)[pix] / 255.0;
    }
};
struct PcGreyF32 {
    static __device__ __forceinline__ double val(const void *__restrict__ src, size_t pix) {
        return (double)static_cast<const float *>(src)[pix];
    }
};
struct PcRgbU8 {
    static __device__ __forceinline__ double val(const void *__restrict__ src, size_t pix) {
        const uint8_t *p = static_cast<const uint8_t *>(src) + pix * 3;
        return ((0.2989 * (double)p[0] + 0.587 * (double)p[1]) + 0.114 * (double)p[2]) / 255.0;
    }
};

template <typename Src>
__device__ __forceinline__ double pc_tap(const void *__restrict__ src, const uint8_t *__restrict__ mask, size_t frame,
                                         int H, int W, int u, int v) {
    if (u < 0 || u >= W || v < 0 || v >= H) return 0.0;
    const size_t pix = frame + (size_t)v * W + u;
    if (mask && mask[pix] == 0) return 0.0;
    return Src::val(src, pix);
}

template <typename Src>
__global__ __launch_bounds__(256) void k_pair_warp(const void *__restrict__ src, const uint8_t *__restrict__ mask, int N,
                                                   int H, int W, const int32_t *__restrict__ frames,
                                                   const double *__restrict__ inv, int S, int tiles_x,
                                                   float *__restrict__ out, uint8_t *__restrict__ cells) {
    __shared__ unsigned long long wave_bits[4];
    const int q = blockIdx.x / tiles_x, tile = blockIdx.x - q * tiles_x;
    const int x = tile * PC_BX + threadIdx.x, y = blockIdx.y * PC_BY + threadIdx.y;      // y < S: S is a multiple of 8
    const int f = frames[q];
    const bool live = x < S && f >= 0 && f < N;
    float res = 0.0f;
    bool seen = false;
    if (live) {
        const double *m = inv + (size_t)q * 6;
        const double xd = (double)x, yd = (double)y;
        const double sx = (m[0] * xd + m[1] * yd) + m[2], sy = (m[3] * xd + m[4] * yd) + m[5];
        const size_t frame = (size_t)f * H * W;
        if (sx >= -1.0 && sx < (double)W && sy >= -1.0 && sy < (double)H) {
            const double xf = floor(sx), yf = floor(sy);
            const double fx = sx - xf, fy = sy - yf;
            const int x0 = (int)xf, y0 = (int)yf;
            const double v00 = pc_tap<Src>(src, mask, frame, H, W, x0, y0);
            const double v10 = pc_tap<Src>(src, mask, frame, H, W, x0 + 1, y0);
            const double v01 = pc_tap<Src>(src, mask, frame, H, W, x0, y0 + 1);
            const double v11 = pc_tap<Src>(src, mask, frame, H, W, x0 + 1, y0 + 1);
            const double top = v00 * (1.0 - fx) + v10 * fx, bot = v01 * (1.0 - fx) + v11 * fx;
            res = (float)(top * (1.0 - fy) + bot * fy);
        }
        if (cells) {
            const double nx = sx + 0.5, ny = sy + 0.5;
            if (nx >= 0.0 && nx < (double)W && ny >= 0.0 && ny < (double)H) {
                const int nu = (int)floor(nx), nv = (int)floor(ny);
                seen = !mask || mask[frame + (size_t)nv * W + nu] != 0;
            }
        }
    }
    if (x < S) out[((size_t)q * S + y) * S + x] = res;
    if (!cells) return;                                    // the same in every thread
    const int tid = threadIdx.y * PC_BX + threadIdx.x;
    const unsigned long long bits = __ballot(seen);        // lane l of wave w: column l & 31, row 2 w + (l >> 5)
    if ((tid & 63) == 0) wave_bits[tid >> 6] = bits;
    __syncthreads();
    if (tid < 4) {
        const int cx = tile * (PC_BX / 8) + tid;
        if (cx < S / 8) {
            const unsigned long long all = (wave_bits[0] | wave_bits[1]) | (wave_bits[2] | wave_bits[3]);
            const unsigned long long cell = 0x000000ff000000ffull << (8 * tid);
            cells[((size_t)q * (S / 8) + blockIdx.y) * (S / 8) + cx] = (all & cell) ? 1 : 0;
        }
    }
}

}  // namespace nof

using namespace nof;

extern "C" {

int nof_mask_roi(const nof_mask_roi_desc *d, void *stream) {
    const char *fn = "mask_roi";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (d->N < 0 || d->N > 65535) return set_error(NOF_EINVAL, "%s: N=%d must be in 0..65535", fn, d->N);
    if (d->H < 1 || d->W < 1) return set_error(NOF_EINVAL, "%s: H=%d, W=%d must be at least 1", fn, d->H, d->W);
    if ((int64_t)d->N * d->H * d->W >= (1ll << 31))
        return set_error(NOF_EINVAL, "%s: N*H*W=%lld must be below 2^31", fn, (long long)d->N * d->H * d->W);
    if (div_up(d->H, ROI_ROWS) > 65535)
        return set_error(NOF_EINVAL, "%s: H=%d must be at most %d", fn, d->H, 65535 * ROI_ROWS);
    if (d->N == 0) return NOF_OK;
    if (int rc = require_pointers(fn, {{d->masks, "masks"}, {d->roi, "roi"}, {d->count, "count"}})) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mask_roi_init, dim3(div_up(d->N, 256)), dim3(256), 0, s, d->roi, d->count, d->N, d->H, d->W);
    if (int rc = check_launch(fn)) return rc;
    hipLaunchKernelGGL(k_mask_roi, dim3(div_up(d->W, ROI_BX), div_up(d->H, ROI_ROWS), (unsigned)d->N), dim3(ROI_BX, ROI_BY),
                       0, s, d->masks, d->H, d->W, d->roi, d->count);
    return check_launch(fn);
}

int nof_warp_images(const nof_warp_images_desc *d, void *stream) {
    const char *fn = "warp_images";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (d->N < 1 || d->N > 65535) return set_error(NOF_EINVAL, "%s: N=%d must be in 1..65535", fn, d->N);
    if (d->H < 1 || d->W < 1) return set_error(NOF_EINVAL, "%s: H=%d, W=%d must be at least 1", fn, d->H, d->W);
    if ((int64_t)d->N * d->H * d->W >= (1ll << 31))
        return set_error(NOF_EINVAL, "%s: N*H*W=%lld must be below 2^31", fn, (long long)d->N * d->H * d->W);
    if (d->format != NOF_WARP_GREY_U8 && d->format != NOF_WARP_GREY_F32 && d->format != NOF_WARP_RGB_U8)
        return set_error(NOF_EINVAL, "%s: format=%d is not one of NOF_WARP_GREY_U8, NOF_WARP_GREY_F32, NOF_WARP_RGB_U8", fn,
                         d->format);
    if (d->S < 8 || d->S > PC_MAX_SIDE || d->S % 8 != 0)
        return set_error(NOF_EINVAL, "%s: S=%d must be a multiple of 8 in 8..%d", fn, d->S, PC_MAX_SIDE);
    const int tiles_x = (int)div_up(d->S, PC_BX);
    if (d->Q < 0 || (int64_t)d->Q * tiles_x >= (1ll << 31))
        return set_error(NOF_EINVAL, "%s: Q=%d must be at least 0 with Q*ceil(S/32) below 2^31", fn, d->Q);
    if (d->Q == 0) return NOF_OK;
    if (int rc = require_pointers(fn, {{d->images, "images"}, {d->frames, "frames"}, {d->inv, "inv"}, {d->out, "out"}}))
        return rc;
    const dim3 grid((unsigned)d->Q * (unsigned)tiles_x, (unsigned)(d->S / PC_BY)), block(PC_BX, PC_BY);
    hipStream_t s = (hipStream_t)stream;
#define PC_LAUNCH(SRC)                                                                                                  \
    hipLaunchKernelGGL(k_pair_warp<SRC>, grid, block, 0, s, d->images, d->masks, d->N, d->H, d->W, d->frames, d->inv, d->S, \
                       tiles_x, d->out, d->cells)
    if (d->format == NOF_WARP_GREY_U8) PC_LAUNCH(PcGreyU8);
    else if (d->format == NOF_WARP_GREY_F32) PC_LAUNCH(PcGreyF32);
    else PC_LAUNCH(PcRgbU8);
#undef PC_LAUNCH
    return check_launch(fn);
}

}  // extern "C"
