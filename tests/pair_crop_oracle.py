"""numpy float64 restatement of csrc/pair_crop.hip's header comment (k_mask_roi, k_pair_warp with cells), and
the shared inputs of tests/test_pair_crop_cpu.py and tests/test_gpu_pair_crop.py. numpy evaluates every
elementwise operation on its own, so the order written here is the order computed and nothing is contracted."""
import numpy as np

GREY_U8, GREY_F32, RGB_U8 = "grey_u8", "grey_f32", "rgb_u8"


def mask_roi(masks):
    """masks [N,H,W] -> (roi [N,4] i32 = umin, umax, vmin, vmax; count [N] i32); empty: (W, -1, H, -1), 0."""
    m = np.asarray(masks) != 0
    N, H, W = m.shape
    roi = np.empty((N, 4), np.int32)
    count = np.empty(N, np.int32)
    for f in range(N):
        v, u = np.nonzero(m[f])
        count[f] = len(u)
        roi[f] = (u.min(), u.max(), v.min(), v.max()) if len(u) else (W, -1, H, -1)
    return roi, count


def mask_roi_brute(mask):
    """Frame::updateRoi's double loop on one [H,W] mask, with the empty case of this project."""
    H, W = mask.shape
    umin, umax, vmin, vmax, n = W, -1, H, -1, 0
    for h in range(H):
        for w in range(W):
            if mask[h, w] > 0:
                umin, umax, vmin, vmax, n = min(umin, w), max(umax, w), min(vmin, h), max(vmax, h), n + 1
    return (umin, umax, vmin, vmax), n


def _values(images, form):
    a = np.asarray(images)
    if form == GREY_U8:
        assert a.dtype == np.uint8 and a.ndim == 3
        return a.astype(np.float64) / 255.0
    if form == GREY_F32:
        assert a.dtype == np.float32 and a.ndim == 3
        return a.astype(np.float64)
    assert form == RGB_U8 and a.dtype == np.uint8 and a.ndim == 4 and a.shape[3] == 3
    a = a.astype(np.float64)
    return ((0.2989 * a[..., 0] + 0.587 * a[..., 1]) + 0.114 * a[..., 2]) / 255.0


def form_of(images):
    a = np.asarray(images)
    return RGB_U8 if a.ndim == 4 else (GREY_U8 if a.dtype == np.uint8 else GREY_F32)


def warp(images, inv, frames, S, masks=None, form=None):
    """-> (crops [Q,S,S] f32, cells [Q,S/8,S/8] u8), as k_pair_warp defines them."""
    val = _values(images, form or form_of(images))
    N, H, W = val.shape
    keep = None if masks is None else (np.asarray(masks) != 0)
    inv = np.asarray(inv, np.float64)
    Q = len(frames)
    out = np.zeros((Q, S, S), np.float32)
    cells = np.zeros((Q, S // 8, S // 8), np.uint8)
    y, x = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    for q in range(Q):
        f = int(frames[q])
        if f < 0 or f >= N:
            continue
        m = inv[q]
        sx = (m[0, 0] * x + m[0, 1] * y) + m[0, 2]
        sy = (m[1, 0] * x + m[1, 1] * y) + m[1, 2]
        with np.errstate(invalid="ignore"):
            near = (sx >= -1.0) & (sx < float(W)) & (sy >= -1.0) & (sy < float(H))
        sxc, syc = np.where(near, sx, 0.0), np.where(near, sy, 0.0)
        xf, yf = np.floor(sxc), np.floor(syc)
        fx, fy = sxc - xf, syc - yf
        x0, y0 = xf.astype(np.int64), yf.astype(np.int64)

        def tap(u, v):
            inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
            uc, vc = np.clip(u, 0, W - 1), np.clip(v, 0, H - 1)
            if keep is not None:
                inside = inside & keep[f, vc, uc]
            return np.where(inside, val[f, vc, uc], 0.0)

        top = tap(x0, y0) * (1.0 - fx) + tap(x0 + 1, y0) * fx
        bot = tap(x0, y0 + 1) * (1.0 - fx) + tap(x0 + 1, y0 + 1) * fx
        res = top * (1.0 - fy) + bot * fy
        out[q] = np.where(near, res, 0.0).astype(np.float32)

        nx, ny = sx + 0.5, sy + 0.5
        with np.errstate(invalid="ignore"):
            seen = (nx >= 0.0) & (nx < float(W)) & (ny >= 0.0) & (ny < float(H))
        nu = np.floor(np.where(seen, nx, 0.0)).astype(np.int64)
        nv = np.floor(np.where(seen, ny, 0.0)).astype(np.int64)
        if keep is not None:
            seen = seen & keep[f, nv, nu]
        cells[q] = seen.reshape(S // 8, 8, S // 8, 8).any(axis=(1, 3))
    return out, cells


# ---- shared inputs -------------------------------------------------------------------------------------

H_ROI, W_ROI = 37, 53          # the ROI-only frame: neither a multiple of the 64 x 32 block


def roi_masks():
    """name -> [37,53] u8 mask: empty, full, one pixel in each corner, two disjoint blobs."""
    H, W = H_ROI, W_ROI
    out = {"empty": np.zeros((H, W), np.uint8), "full": np.full((H, W), 255, np.uint8)}
    for name, (v, u) in {"corner_tl": (0, 0), "corner_tr": (0, W - 1), "corner_bl": (H - 1, 0),
                         "corner_br": (H - 1, W - 1)}.items():
        out[name] = np.zeros((H, W), np.uint8)
        out[name][v, u] = 1
    blobs = np.zeros((H, W), np.uint8)
    blobs[3:9, 5:11] = 7
    blobs[20:31, 33:47] = 200
    out["blobs"] = blobs
    return out


H_IMG, W_IMG, N_IMG = 48, 64, 3


def sources(seed=5):
    """form -> [3,48,64(,3)] images of smooth texture plus noise, and [3,48,64] u8 masks (a disc, an
    off-centre box, and an empty mask)."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(H_IMG), np.arange(W_IMG), indexing="ij")
    rgb = np.empty((N_IMG, H_IMG, W_IMG, 3), np.uint8)
    for f in range(N_IMG):
        for c in range(3):
            wave = 110 + 70 * np.sin(0.23 * (f + 1) * u + c) * np.cos(0.17 * (c + 1) * v - f)
            rgb[f, ..., c] = np.clip(wave + rng.integers(-30, 31, (H_IMG, W_IMG)), 0, 255).astype(np.uint8)
    grey_u8 = rgb[..., 1].copy()
    grey_f32 = (rng.random((N_IMG, H_IMG, W_IMG)) * 0.5 + grey_u8 / 510.0).astype(np.float32)
    masks = np.zeros((N_IMG, H_IMG, W_IMG), np.uint8)
    masks[0] = ((u - 30) ** 2 + (v - 22) ** 2 <= 15 ** 2) * 255
    masks[1, 9:40, 20:58] = 1
    return {GREY_U8: grey_u8, GREY_F32: grey_f32, RGB_U8: rgb}, masks


def scale2_inverse(ox, oy):
    """The inverse of a scale-2 transform onto integer offsets: crop (x, y) reads source (x / 2 + ox, y / 2 + oy)."""
    return np.array([[0.5, 0.0, float(ox)], [0.0, 0.5, float(oy)]])


def warp_cases(S):
    """(inv [6,2,3], frames [6]): identity; the exact scale-2 case; 33 degrees at scale 1.7; wholly outside
    the image; a down-scale of 0.4; and a crop whose frame index 7 does not exist. Frame 1 is used three times."""
    c, s = np.cos(np.radians(33.0)), np.sin(np.radians(33.0))
    rot = np.array([[c / 1.7, s / 1.7, 20.0 - 0.2 * S], [-s / 1.7, c / 1.7, 14.0 + 0.1 * S]])
    inv = np.stack([np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]),
                    scale2_inverse(6, 4),
                    rot,
                    np.array([[1.0, 0.0, 500.0], [0.0, 1.0, -900.0]]),
                    np.array([[2.5, 0.0, -7.3], [0.0, 2.5, -11.9]]),
                    np.array([[1.0, 0.0, 3.0], [0.0, 1.0, 2.0]])])
    frames = np.array([0, 1, 1, 2, 1, 7], np.int32)
    return inv, frames
