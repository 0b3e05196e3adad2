"""Pair crops on the device, and find_corres: from frames, masks, poses and frame pairs to 3-D matches.

The reference never shows LoFTR a whole frame. GluNet::getProcessedImagePairs -> processImagePair
(BundleTrack/src/FeatureManager.cpp) takes each frame's mask bounding box (Frame::updateRoi), rotates frame
B in the image plane into frame A's orientation (Utils::getRotateImageTransform), pads both boxes, brings
them to a common scale and warps both masked grey images to a square of feature_corres.resize pixels; the
matches are carried back through the two transforms. Here mask_roi and warp_images are the two calls of
include/nof.h group 15 (csrc/pair_crop.hip, whose header comment is the definition), rotate_image_transform,
pair_transforms and invert_affine restate the reference's host arithmetic in numpy float64, pair_crops chains
them with one host read, and find_corres composes pair_crops, Loftr.match, FineMatches.to_pixels,
lift_matches and ransac_pairs.

No CPU fallback: mask_roi, warp_images, pair_crops and find_corres raise if libnof.so cannot run.
"""
import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._args import as_host, as_tensor, default_device

__all__ = ["mask_roi", "rotate_image_transform", "rotation_about_axis_z", "pair_transforms", "invert_affine",
           "warp_images", "pair_crops", "find_corres", "PairCrops", "Correspondences", "CELL", "MAX_SIDE", "TILE"]

CELL = 8                # crop pixels per side of a coarse cell
MAX_SIDE = 4096         # PC_MAX_SIDE of csrc/pair_crop.hip
TILE = (8, 32)          # PC_BY, PC_BX: the rows and columns of crop pixels one block takes


@dataclass
class PairCrops:
    """One pair_crops call. Crop A of pair p is images[2p], crop B images[2p+1]."""
    images: torch.Tensor                # [2P,S,S] f32 in 0..1, device
    cells: Optional[torch.Tensor]       # [2P,S/8,S/8] u8, device; None without cell_masks
    match_pairs: np.ndarray             # [P,2] i64 = (2p, 2p+1)
    tf_a: np.ndarray                    # [P,3,3] f64, frame A pixel -> crop pixel
    tf_b: np.ndarray                    # [P,3,3] f64
    valid: np.ndarray                   # [P] bool: both frames have foreground
    roi: torch.Tensor                   # [N,4] i32 (umin, umax, vmin, vmax), device
    count: torch.Tensor                 # [N] i32 foreground pixels, device


@dataclass
class Correspondences:
    """One find_corres call. Rows are ordered by pair; uv_* are in the frames' own pixels."""
    crops: PairCrops
    fine: object                        # the FineMatches of the crops
    uv_a: torch.Tensor                  # [M,2] f64
    uv_b: torch.Tensor                  # [M,2] f64
    pair_start: torch.Tensor            # [P+1] i32 over the M rows
    conf: torch.Tensor                  # [M] f32
    n_raw: torch.Tensor                 # [P] i32: matches per pair before the lift
    lifted: object                      # LiftedMatches.compact(): the rows with depth on both sides
    ransac: Optional[object]            # RansacResult over lifted's rows, or None


def _check_sizes(what, out_size, margin):
    if isinstance(out_size, bool) or not isinstance(out_size, (int, np.integer)):
        raise ValueError(f"{what}: out_size={out_size!r} must be an integer")
    if out_size < CELL or out_size > MAX_SIDE or out_size % CELL != 0:
        raise ValueError(f"{what}: out_size={out_size} must be a multiple of {CELL} in {CELL} .. {MAX_SIDE}")
    if margin is not None:
        if isinstance(margin, bool) or not isinstance(margin, (int, np.integer)):
            raise ValueError(f"{what}: margin={margin!r} must be an integer")
        if margin < 1:
            raise ValueError(f"{what}: margin={margin} must be at least 1")
    return int(out_size), None if margin is None else int(margin)


def _masks_u8(masks, what):
    """masks (array or tensor, [H,W] or [N,H,W], bool or integer) -> ([N,H,W] u8 tensor, 1 = foreground, single)."""
    t = as_tensor(masks)
    if t.dim() not in (2, 3):
        raise ValueError(f"{what}: masks must be [H,W] or [N,H,W], got {tuple(t.shape)}")
    if t.is_floating_point() or t.is_complex():
        raise ValueError(f"{what}: masks must be bool or an integer type, got {t.dtype}")
    single = t.dim() == 2
    t = t[None] if single else t
    N, H, W = t.shape
    if N > 65535 or H < 1 or W < 1 or N * H * W >= 2 ** 31:
        raise ValueError(f"{what}: masks of {N}x{H}x{W} (N at most 65535, H, W at least 1, N*H*W < 2^31)")
    return (t != 0).to(torch.uint8).contiguous(), single


def _mask_roi(L, m):
    N, H, W = m.shape
    roi = torch.empty((N, 4), dtype=torch.int32, device=m.device)
    count = torch.empty(N, dtype=torch.int32, device=m.device)
    D = _lib.MaskRoiDesc()
    D.masks, D.N, D.H, D.W, D.roi, D.count = _lib.ptr(m), N, H, W, _lib.ptr(roi), _lib.ptr(count)
    _lib.check(L.nof_mask_roi(ctypes.byref(D), _lib.stream_of(m)), "mask_roi")
    return roi, count


def mask_roi(masks, device=None):
    """Frame::updateRoi for N frames at once. masks [N,H,W] or one [H,W], numpy or tensor, bool or any
    integer type, non-zero = foreground -> (roi [N,4] i32 = (umin, umax, vmin, vmax), inclusive; count [N]
    i32), device tensors (without N for a single mask). An empty mask gives (W, -1, H, -1) and 0."""
    m, single = _masks_u8(masks, "mask_roi")
    dev = default_device(m, device)
    L = _lib.lib()
    with torch.cuda.device(dev):
        roi, count = _mask_roi(L, m.to(dev))
    return (roi[0], count[0]) if single else (roi, count)


def _compose(A, B):
    """A B for two pixel transforms whose last row is (0, 0, 1), every sum as (x + y) + z."""
    C = np.eye(3)
    for i in range(2):
        C[i, 0] = A[i, 0] * B[0, 0] + A[i, 1] * B[1, 0]
        C[i, 1] = A[i, 0] * B[0, 1] + A[i, 1] * B[1, 1]
        C[i, 2] = (A[i, 0] * B[0, 2] + A[i, 1] * B[1, 2]) + A[i, 2]
    return C


def _translate(tx, ty):
    T = np.eye(3)
    T[0, 2], T[1, 2] = tx, ty
    return T


def _scale(s):
    T = np.eye(3)
    T[0, 0] = T[1, 1] = s
    return T


def _corner_box(tf, corners):
    """(umin, umax, vmin, vmax) of the corners [(u, v), ...] carried through tf."""
    us = [(tf[0, 0] * u + tf[0, 1] * v) + tf[0, 2] for u, v in corners]
    vs = [(tf[1, 0] * u + tf[1, 1] * v) + tf[1, 2] for u, v in corners]
    return min(us), max(us), min(vs), max(vs)


def rotate_image_transform(H, W, rot):
    """Utils::getRotateImageTransform on the identity: the [3,3] f64 transform that moves the image centre
    (W/2, H/2) to the origin, rotates by rot as [[cos, -sin], [sin, cos]], and re-centres by side/2, side =
    the larger extent of the rotated corners (0,0), (W,0), (0,H), (W,H), truncated to an integer."""
    rot = float(rot)
    if not math.isfinite(rot):
        raise ValueError(f"rotate_image_transform: rot={rot} is not finite")
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"rotate_image_transform: H={H}, W={W} must be at least 1")
    F = _translate(-(W / 2.0), -(H / 2.0))
    R = np.eye(3)
    R[0, 0], R[0, 1], R[1, 0], R[1, 1] = math.cos(rot), -math.sin(rot), math.sin(rot), math.cos(rot)
    F = _compose(R, F)
    umin, umax, vmin, vmax = _corner_box(F, [(0, 0), (W, 0), (0, H), (W, H)])
    side = int(max(umax - umin, vmax - vmin))                      # int side = std::max(...): truncation
    return _compose(_translate(side / 2.0, side / 2.0), F)


def rotation_about_axis_z(R):
    """angle * axis_z of the rotation matrix R [3,3]: the z component of its rotation vector, by the route
    of Eigen's AngleAxis::fromRotationMatrix (matrix -> quaternion -> angle, axis), angle in [0, pi]."""
    m = np.asarray(R, np.float64)
    t = (m[0, 0] + m[1, 1]) + m[2, 2]
    q = [0.0, 0.0, 0.0]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        q = [(m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t]
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(((m[i, i] - m[j, j]) - m[k, k]) + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        w = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    n = math.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
    if n == 0.0:
        return 0.0                                                  # angle 0 about (1, 0, 0)
    angle = 2.0 * math.atan2(n, abs(w))
    if w < 0.0:
        n = -n
    return angle * (q[2] / n)


def pair_transforms(roi, poses, pairs, H, W, out_size=400, margin=10):
    """processImagePair's two transforms for P pairs, host only, numpy float64 -> (tf_a [P,3,3], tf_b
    [P,3,3], valid [P] bool); tf maps a frame's pixel to its crop's pixel, last row (0, 0, 1).

    roi [N,4] (umin, umax, vmin, vmax) or [N,5] with count as its last column (mask_roi's outputs; without a
    count, a frame with umax < umin is empty); poses [N,4,4] camera in world; pairs [P,2] = (a, b).
    R_BA = R_a^T R_b, rot = rotation_about_axis_z(R_BA); B is turned by rotate_image_transform(H, W, rot) and
    its ROI replaced by the bounding box of its four turned corners; both boxes are moved to start at
    margin; WA = umax - umin + 2 margin and likewise HA, WB, HB, truncated toward zero; each side is scaled
    by max_dim / max(W?, H?), max_dim the largest of the four, then both by out_size / max_dim. A pair with
    an empty frame is invalid and gets identity transforms."""
    what = "pair_transforms"
    out_size, margin = _check_sizes(what, out_size, margin)
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"{what}: H={H}, W={W} must be at least 1")
    r = as_host(roi, np.int64)
    if r.ndim != 2 or r.shape[1] not in (4, 5):
        raise ValueError(f"{what}: roi must be [N,4] or [N,5], got {r.shape}")
    N = len(r)
    T = as_host(poses, np.float64)
    if T.shape != (N, 4, 4):
        raise ValueError(f"{what}: poses must be [{N},4,4], got {T.shape}")
    if not np.isfinite(T).all():
        raise ValueError(f"{what}: poses is not finite")
    pf = as_host(pairs, np.int64)
    if pf.ndim != 2 or pf.shape[1] != 2:
        raise ValueError(f"{what}: pairs must be [P,2], got {pf.shape}")
    if (pf < 0).any() or (pf >= N).any():
        raise ValueError(f"{what}: pairs has a frame index outside 0 .. {N - 1}")
    empty = (r[:, 4] <= 0) if r.shape[1] == 5 else ((r[:, 1] < r[:, 0]) | (r[:, 3] < r[:, 2]))
    P = len(pf)
    tf_a, tf_b = np.tile(np.eye(3), (P, 1, 1)), np.tile(np.eye(3), (P, 1, 1))
    valid = np.zeros(P, bool)
    for p, (a, b) in enumerate(pf):
        if empty[a] or empty[b]:
            continue
        valid[p] = True
        Ra, Rb = T[a, :3, :3], T[b, :3, :3]
        R_BA = np.empty((3, 3))
        for i in range(3):
            for j in range(3):
                R_BA[i, j] = (Ra[0, i] * Rb[0, j] + Ra[1, i] * Rb[1, j]) + Ra[2, i] * Rb[2, j]
        tfB = rotate_image_transform(H, W, rotation_about_axis_z(R_BA))
        ua0, ua1, va0, va1 = (int(x) for x in r[a, :4])
        ub0, ub1, vb0, vb1 = (int(x) for x in r[b, :4])
        umin, umax, vmin, vmax = _corner_box(tfB, [(ub0, vb0), (ub0, vb1), (ub1, vb0), (ub1, vb1)])
        tfA = _translate(float(-ua0 + margin), float(-va0 + margin))
        tfB = _compose(_translate(-umin + margin, -vmin + margin), tfB)
        WA, HA = ua1 - ua0 + margin * 2, va1 - va0 + margin * 2
        HB, WB = int((vmax - vmin) + margin * 2), int((umax - umin) + margin * 2)      # float -> int: truncation
        max_dim = max(WA, HA, WB, HB)
        tfA = _compose(_scale(float(max_dim) / max(WA, HA)), tfA)
        tfB = _compose(_scale(float(max_dim) / max(WB, HB)), tfB)
        last = _scale(float(out_size) / max_dim)
        tf_a[p], tf_b[p] = _compose(last, tfA), _compose(last, tfB)
    return tf_a, tf_b, valid


def invert_affine(tf):
    """The inverse of affine pixel transforms as [..., 2, 3] f64: tf is [..., 3, 3] with last row (0, 0, 1),
    or [..., 2, 3]. With a b tx / c d ty: det = a d - b c, the linear part (d / det, (-b) / det, (-c) / det,
    a / det) = (i00, i01, i10, i11), and the translation (-(i00 tx + i01 ty), -(i10 tx + i11 ty))."""
    what = "invert_affine"
    M = as_host(tf, np.float64)
    if M.ndim < 2 or M.shape[-2:] not in ((3, 3), (2, 3)):
        raise ValueError(f"{what}: tf must be [...,3,3] or [...,2,3], got {M.shape}")
    if not np.isfinite(M).all():
        raise ValueError(f"{what}: tf is not finite")
    if M.shape[-2] == 3 and (M[..., 2, :] != (0.0, 0.0, 1.0)).any():
        raise ValueError(f"{what}: tf must be affine (last row 0 0 1)")
    a, b, tx, c, d, ty = M[..., 0, 0], M[..., 0, 1], M[..., 0, 2], M[..., 1, 0], M[..., 1, 1], M[..., 1, 2]
    det = a * d - b * c
    if (det == 0.0).any():
        raise ValueError(f"{what}: tf has a singular linear part")
    out = np.empty(M.shape[:-2] + (2, 3))
    out[..., 0, 0], out[..., 0, 1], out[..., 1, 0], out[..., 1, 1] = d / det, (-b) / det, (-c) / det, a / det
    out[..., 0, 2] = -(out[..., 0, 0] * tx + out[..., 0, 1] * ty)
    out[..., 1, 2] = -(out[..., 1, 0] * tx + out[..., 1, 1] * ty)
    if not np.isfinite(out).all():
        raise ValueError(f"{what}: the inverse of tf is not finite")
    return out


def _source(images, what):
    """images -> (contiguous tensor, format, (N, H, W)): [N,H,W] u8, [N,H,W] f32 or [N,H,W,3] u8."""
    t = as_tensor(images)
    if t.dtype == torch.uint8 and t.dim() == 3:
        fmt = _lib.WARP_GREY_U8
    elif t.dtype == torch.float32 and t.dim() == 3:
        fmt = _lib.WARP_GREY_F32
    elif t.dtype == torch.uint8 and t.dim() == 4 and t.shape[3] == 3:
        fmt = _lib.WARP_RGB_U8
    else:
        raise ValueError(f"{what}: images must be [N,H,W] uint8, [N,H,W] float32 or [N,H,W,3] uint8, got "
                         f"{tuple(t.shape)} {t.dtype}")
    N, H, W = t.shape[:3]
    if N < 1 or N > 65535 or H < 1 or W < 1 or N * H * W >= 2 ** 31:
        raise ValueError(f"{what}: images of {N}x{H}x{W} (N in 1 .. 65535, H, W at least 1, N*H*W < 2^31)")
    return t.contiguous(), fmt, (N, H, W)


def _warp(L, src, fmt, shape, m, inv, frames, S, cell_masks):
    N, H, W = shape
    dev = src.device
    Q = len(frames)
    out = torch.empty((Q, S, S), dtype=torch.float32, device=dev)
    cells = torch.empty((Q, S // CELL, S // CELL), dtype=torch.uint8, device=dev) if cell_masks else None
    if Q:
        fd, vd = torch.from_numpy(frames).to(dev), torch.from_numpy(inv).to(dev)
        D = _lib.WarpImagesDesc()
        D.images, D.masks, D.N, D.H, D.W, D.format = _lib.ptr(src), _lib.ptr(m), N, H, W, fmt
        D.frames, D.inv, D.Q, D.S, D.out, D.cells = _lib.ptr(fd), _lib.ptr(vd), Q, S, _lib.ptr(out), _lib.ptr(cells)
        _lib.check(L.nof_warp_images(ctypes.byref(D), _lib.stream_of(src)), "warp_images")
    return out, cells


def _warp_args(what, inv, frames, shape, masks):
    inv = as_host(inv, np.float64)
    if inv.ndim != 3 or inv.shape[1:] != (2, 3):
        raise ValueError(f"{what}: inv must be [Q,2,3], got {inv.shape}")
    if not np.isfinite(inv).all():
        raise ValueError(f"{what}: inv is not finite")
    fr = as_host(frames, np.int64).reshape(-1)
    if len(fr) != len(inv):
        raise ValueError(f"{what}: frames has {len(fr)} entries, inv {len(inv)}")
    fr = np.ascontiguousarray(np.clip(fr, -1, 2 ** 31 - 1).astype(np.int32))      # any frame outside 0 .. N-1 gives zeros
    m = None
    if masks is not None:
        m, _ = _masks_u8(masks, what)
        if tuple(m.shape) != tuple(shape):
            raise ValueError(f"{what}: masks is {tuple(m.shape)}, images {tuple(shape)}")
    return inv, fr, m


def warp_images(images, inv, frames, out_size, masks=None, cell_masks=True):
    """Q square crops of side out_size in one launch -> (crops [Q,S,S] f32 in 0..1, cells [Q,S/8,S/8] u8 or
    None), device tensors. images: [N,H,W] uint8 grey, [N,H,W] float32 grey in 0..1 or [N,H,W,3] uint8 RGB
    (grey per tap with to_grey's weights). Crop q reads frame frames[q] through inv[q], the [2,3] f64 affine
    map from crop pixel to source pixel (invert_affine of a pair transform), bilinear in float64; a tap
    outside the image or where masks [N,H,W] is 0 reads 0. A frames[q] outside 0 .. N-1 gives a crop of
    zeros. cells is 1 for each 8 x 8 cell with a pixel whose nearest source pixel is inside the image and the
    mask: what Loftr.match takes as masks."""
    what = "warp_images"
    S, _ = _check_sizes(what, out_size, None)
    src, fmt, shape = _source(images, what)
    inv, fr, m = _warp_args(what, inv, frames, shape, masks)
    dev = default_device(src)
    L = _lib.lib()
    with torch.cuda.device(dev):
        return _warp(L, src.to(dev), fmt, shape, None if m is None else m.to(dev), inv, fr, S, bool(cell_masks))


def pair_crops(images, masks, poses, pairs, out_size=400, margin=10, cell_masks=True):
    """processImagePair for P pairs -> PairCrops: mask_roi, one host read of [N,5] int32 (ROI and count),
    pair_transforms on the host, and one warp_images launch for all 2P crops (crop A of pair p at 2p, crop B
    at 2p+1). images as warp_images takes them, masks [N,H,W] (non-zero = object), poses [N,4,4] camera in
    world, pairs [P,2] = (a, b). The crops of an invalid pair (a frame without foreground) are zeros, their
    cells 0 and their transforms the identity."""
    what = "pair_crops"
    S, margin = _check_sizes(what, out_size, margin)
    src, fmt, shape = _source(images, what)
    N, H, W = shape
    m, _ = _masks_u8(masks, what)
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"{what}: masks is {tuple(m.shape)}, images {tuple(shape)}")
    dev = default_device(src)
    L = _lib.lib()
    with torch.cuda.device(dev):
        src, m = src.to(dev), m.to(dev)
        roi, count = _mask_roi(L, m)
        host = torch.cat([roi, count[:, None]], 1).cpu().numpy()                   # the one host read
        tf_a, tf_b, valid = pair_transforms(host, poses, pairs, H, W, S, margin)
        pf = as_host(pairs, np.int64)
        P = len(pf)
        inv = invert_affine(np.stack([tf_a, tf_b], 1).reshape(2 * P, 3, 3))
        frames = np.where(valid[:, None], pf, -1).reshape(2 * P).astype(np.int32)
        crops, cells = _warp(L, src, fmt, shape, m, np.ascontiguousarray(inv), np.ascontiguousarray(frames), S,
                             bool(cell_masks))
    match_pairs = np.arange(2 * P, dtype=np.int64).reshape(P, 2)
    return PairCrops(images=crops, cells=cells, match_pairs=match_pairs, tf_a=tf_a, tf_b=tf_b, valid=valid, roi=roi,
                     count=count)


def find_corres(matcher, images, masks, maps, poses, pairs, *, out_size=400, margin=10, thr=0.2, border_rm=2,
                temperature=0.1, cell_masks=True, max_dist=None, max_normal_deg=None, ransac=None):
    """From frames to RANSAC-filtered 3-D matches in one call -> Correspondences. matcher is a Loftr, maps the
    FrameMaps of the frames (prepare_frames), ransac None or the keyword arguments of ransac_pairs (at least
    inlier_dist). It is this composition and nothing else:

        pc = pair_crops(images, masks, poses, pairs, out_size, margin, cell_masks)
        fm = matcher.match(pc.images, pc.match_pairs, pc.cells if cell_masks else None, thr=thr,
                           border_rm=border_rm, temperature=temperature)
        uv_a, uv_b, pair_start, conf = fm.to_pixels(scale=8, tf_a=pc.tf_a, tf_b=pc.tf_b)
        lifted = lift_matches(maps, pairs, uv_a, uv_b, pair_start, poses=poses, max_dist=max_dist,
                              max_normal_deg=max_normal_deg).compact()
        res = ransac_pairs(lifted.pts_a, lifted.pts_b, lifted.pair_start, lifted.normals_a, lifted.normals_b,
                           conf=conf[lifted.rows].double(), **ransac)

    n_raw [P] is the number of matches per pair before the lift, the figure the reference's find_corres
    compares with min_match_with_ref. cell_masks=False runs LoFTR without a cell mask, as the reference does;
    the default keeps background cells out of the dual softmax."""
    from .frames import lift_matches
    from .ransac import ransac_pairs
    what = "find_corres"
    if ransac is not None and not isinstance(ransac, dict):
        raise ValueError(f"{what}: ransac must be None or a dict of ransac_pairs' keyword arguments")
    if len(as_host(pairs, np.int64).reshape(-1, 2)) < 1:
        raise ValueError(f"{what}: pairs must hold at least one pair")
    pc = pair_crops(images, masks, poses, pairs, out_size, margin, cell_masks)
    fm = matcher.match(pc.images, pc.match_pairs, pc.cells if cell_masks else None, thr=thr, border_rm=border_rm,
                       temperature=temperature)
    uv_a, uv_b, pair_start, conf = fm.to_pixels(scale=8, tf_a=pc.tf_a, tf_b=pc.tf_b)
    lifted = lift_matches(maps, pairs, uv_a, uv_b, pair_start, poses=poses, max_dist=max_dist,
                          max_normal_deg=max_normal_deg).compact()
    res = None
    if ransac is not None:
        res = ransac_pairs(lifted.pts_a, lifted.pts_b, lifted.pair_start, lifted.normals_a, lifted.normals_b,
                           conf=conf[lifted.rows].double(), **ransac)
    return Correspondences(crops=pc, fine=fm, uv_a=uv_a, uv_b=uv_b, pair_start=pair_start, conf=conf,
                           n_raw=pair_start[1:] - pair_start[:-1], lifted=lifted, ransac=res)
