"""Pose-graph optimisation on the device: sparse matches plus dense projective ICP.

The step the reference runs once per incoming frame over a window of key frames
(Bundler::optimizeGPU -> OptimizerGpu::optimizeFrames -> SBA::align -> CUDASolverBundling): a fixed
number of Gauss-Newton steps over camera-in-world poses, each with a Jacobi-preconditioned
conjugate-gradient solve. Here it is nof_pose_graph_optimize (csrc/pose_graph.hip, include/nof.h
group 9): float64 in a stated order, no floating-point atomics, the same bytes on every run, every
launch on the caller's stream and nothing read back until the call is over. The definition is the
header comment of csrc/pose_graph.hip; tests/pose_graph_oracle.py restates it in numpy.

No CPU fallback: optimize_poses raises if libnof.so cannot run. Every argument is validated before
the first device call.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._args import as_host, as_tensor, default_device

__all__ = ["optimize_poses", "MAX_FRAMES", "MAX_RADIUS", "ROW_TILE"]

MAX_FRAMES = 128        # PG_MAX_FRAMES of csrc/pose_graph.hip
MAX_RADIUS = 32         # PG_MAX_RADIUS
ROW_TILE = 256          # PG_TILE: sparse rows, or source pixels, a block takes at a time


def _tensor(a, dtype, name, shape):
    """a (array or tensor) as a contiguous tensor of dtype on the device it came from; shape has None
    for a free dimension."""
    t = as_tensor(a)
    if t.dim() != len(shape) or any(s is not None and s != g for s, g in zip(shape, t.shape)):
        want = ",".join("*" if s is None else str(s) for s in shape)
        raise ValueError(f"optimize_poses: {name} must be [{want}], got {tuple(t.shape)}")
    return t.to(dtype).contiguous()


def optimize_poses(poses, *, pair_frames=None, pts_a=None, pts_b=None, pair_start=None, weight=None,
                   points=None, normals=None, K=None, fixed=None, n_outer=7, n_inner=5, robust_delta=0.005,
                   w_sparse=1.0, w_dense=1.0, dist_thresh=0.01, normal_thresh=math.cos(math.radians(20.0)),
                   depth_min=0.1, depth_max=9999.0, radius=5, max_rot_deg=60.0, return_debug=False, device=None):
    """Optimise the camera-in-world poses [N,4,4] (float64, array or tensor) of a window of frames ->
    (poses [N,4,4], history [n_outer+1,4]) as device tensors; with return_debug a dict comes third.

    Sparse term: pair_frames [P,2] names the frames (i, j) of each pair, pts_a / pts_b [M,3] are the
    matched points in the cameras of i and j, concatenated per pair with pair_start [P+1] (the layout
    ransac_pairs takes and returns); weight [M] of any dtype, 0 drops a row, so weight=result.inlier
    feeds a RansacResult in without compaction. Dense term: points / normals [N,H,W,3] float32
    camera-space maps at the resolution of K [3,3]. Either term may be absent, not both.

    fixed [N] bool (default: frame 0 only) marks constants; at least one frame must be fixed.
    history rows: sparse energy, dense energy, live sparse rows, dense correspondences, at each of the
    n_outer linearisations and at the final poses. n_outer and n_inner are fixed counts: there is no
    early exit.

    Defaults of the reference: n_outer, n_inner, robust_delta, radius and max_rot_deg are bundle.
    num_iter_outter, num_iter_inner, robust_delta, depth_association_radius and icp_pose_rot_thres
    (BundleTrack/config_ho3d.yml:35, 36, 49, 40, 43); dist_thresh and normal_thresh are p2p.max_dist
    and cos(p2p.max_normal_angle) (config_ho3d.yml:100-101, read at CUDASolverBundling.cu:101-102);
    depth_min and depth_max are CUDASolverBundling.cu:108-109.

    return_debug: iter_poses [n_outer+1,N,4,4], A [n_outer,6N,6N], g [n_outer,6N], delta [n_outer,6N]
    and, with a dense term, dense_index [n_outer,N,N,H*W] int32: the target pixel chosen for (target i,
    source j, source pixel), -1 where there is none or the ordered pair is not active."""
    what = "optimize_poses"
    T = _tensor(poses, torch.float64, "poses", (None, 4, 4))
    N = T.shape[0]
    if N < 1 or N > MAX_FRAMES:
        raise ValueError(f"{what}: N={N} frames (1 .. {MAX_FRAMES})")
    sparse = pair_frames is not None
    dense = points is not None or normals is not None
    if not sparse and not dense:
        raise ValueError(f"{what}: neither the sparse term (pair_frames, pts_a, pts_b) nor the dense term "
                         "(points, normals, K) is given")
    n_outer, n_inner, radius = int(n_outer), int(n_inner), int(radius)
    if n_outer < 1 or n_outer > 1024 or n_inner < 0 or n_inner > 1024:
        raise ValueError(f"{what}: n_outer={n_outer} (1 .. 1024), n_inner={n_inner} (0 .. 1024)")
    if not float(robust_delta) > 0:
        raise ValueError(f"{what}: robust_delta={robust_delta} must be positive")
    fx = np.zeros(N, bool)
    if fixed is None:
        fx[0] = True
    else:
        f = as_host(fixed)
        if f.shape != (N,):
            raise ValueError(f"{what}: fixed must be [{N}], got {f.shape}")
        fx = f.astype(bool)
    if not fx.any():
        raise ValueError(f"{what}: no frame is fixed, the gauge is free")

    pf = a = b = ps = w = None
    P = M = 0
    if sparse:
        if pts_a is None or pts_b is None:
            raise ValueError(f"{what}: pair_frames needs pts_a and pts_b")
        pf_h = as_host(pair_frames, np.int64)
        if pf_h.ndim != 2 or pf_h.shape[1] != 2:
            raise ValueError(f"{what}: pair_frames must be [P,2], got {pf_h.shape}")
        P = len(pf_h)
        if P < 1 or P > 65535:
            raise ValueError(f"{what}: {P} pairs (1 .. 65535)")
        if (pf_h < 0).any() or (pf_h >= N).any():
            raise ValueError(f"{what}: pair_frames has a frame index outside 0 .. {N - 1}")
        if (pf_h[:, 0] == pf_h[:, 1]).any():
            raise ValueError(f"{what}: pair_frames has a pair of a frame with itself")
        a, b = _tensor(pts_a, torch.float64, "pts_a", (None, 3)), _tensor(pts_b, torch.float64, "pts_b", (None, 3))
        M = len(a)
        if len(b) != M:
            raise ValueError(f"{what}: pts_a has {M} rows, pts_b {len(b)}")
        if M >= 2 ** 31:
            raise ValueError(f"{what}: {M} rows (max 2^31 - 1)")
        if pair_start is None:
            if P != 1:
                raise ValueError(f"{what}: pair_start is needed for {P} pairs")
            ps_h = np.array([0, M], np.int64)
        else:
            ps_h = as_host(pair_start, np.int64).reshape(-1)
        if ps_h.shape != (P + 1,) or ps_h[0] != 0 or ps_h[-1] != M or (np.diff(ps_h) < 0).any():
            raise ValueError(f"{what}: pair_start must be [{P + 1}], start at 0, never decrease and end at M={M}")
        if weight is not None:
            w = _tensor(weight, torch.float64, "weight", (M,))
            if M and not bool(((w >= 0) & (w < math.inf)).all()):       # also catches NaN
                raise ValueError(f"{what}: weight must be finite and not negative")
        if not float(w_sparse) >= 0:
            raise ValueError(f"{what}: w_sparse={w_sparse} must not be negative")
        pf, ps = torch.from_numpy(pf_h.astype(np.int32)), torch.from_numpy(ps_h.astype(np.int32))
    pm = nm = None
    H = W = 0
    kk = np.zeros(4)
    min_trace = -math.inf
    if dense:
        if points is None or normals is None or K is None:
            raise ValueError(f"{what}: the dense term needs points, normals and K")
        pm = _tensor(points, torch.float32, "points", (N, None, None, 3))
        H, W = int(pm.shape[1]), int(pm.shape[2])
        nm = _tensor(normals, torch.float32, "normals", (N, H, W, 3))
        if H < 1 or W < 1 or H * W >= 2 ** 24:
            raise ValueError(f"{what}: maps of {H}x{W} (at least 1x1, H*W < 2^24)")
        Kh = as_host(K, np.float64)
        if Kh.shape != (3, 3) or not np.isfinite(Kh).all():
            raise ValueError(f"{what}: K must be a finite [3,3], got {Kh.shape}")
        kk = np.array([Kh[0, 0], Kh[1, 1], Kh[0, 2], Kh[1, 2]])
        if radius < 0 or radius > MAX_RADIUS:
            raise ValueError(f"{what}: radius={radius} (0 .. {MAX_RADIUS})")
        if not float(dist_thresh) > 0 or not float(w_dense) >= 0:
            raise ValueError(f"{what}: dist_thresh={dist_thresh} must be positive and w_dense={w_dense} not negative")
        if any(math.isnan(float(v)) for v in (normal_thresh, depth_min, depth_max, max_rot_deg)):
            raise ValueError(f"{what}: normal_thresh, depth_min, depth_max or max_rot_deg is NaN")
        if float(max_rot_deg) < 180.0:
            min_trace = 1.0 + 2.0 * math.cos(math.radians(max(float(max_rot_deg), 0.0)))

    dev = default_device(T, device)
    L = _lib.lib()
    f64 = torch.float64
    n = 6 * N
    with torch.cuda.device(dev):
        T, pf, a, b, ps, w, pm, nm = (None if x is None else x.to(dev).contiguous() for x in (T, pf, a, b, ps, w, pm, nm))
        fixed_d = torch.from_numpy(fx.astype(np.uint8)).to(dev)
        out = torch.zeros((N, 4, 4), dtype=f64, device=dev)
        history = torch.zeros((n_outer + 1, 4), dtype=f64, device=dev)
        nbytes = int(L.nof_pose_graph_workspace_bytes(N, P, M, H, W))
        ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
        dbg = {}
        if return_debug:
            dbg["iter_poses"] = torch.zeros((n_outer + 1, N, 4, 4), dtype=f64, device=dev)
            dbg["A"] = torch.zeros((n_outer, n, n), dtype=f64, device=dev)
            dbg["g"] = torch.zeros((n_outer, n), dtype=f64, device=dev)
            dbg["delta"] = torch.zeros((n_outer, n), dtype=f64, device=dev)
            if dense:
                dbg["dense_index"] = torch.full((n_outer, N, N, H * W), -1, dtype=torch.int32, device=dev)
        D = _lib.PoseGraphDesc()
        D.poses, D.fixed, D.N, D.n_outer, D.n_inner, D.P, D.M = _lib.ptr(T), _lib.ptr(fixed_d), N, n_outer, n_inner, P, M
        D.pair_frames, D.pts_a, D.pts_b, D.pair_start, D.weight = (_lib.ptr(x) for x in (pf, a, b, ps, w))
        D.points, D.normals, D.H, D.W, D.radius = _lib.ptr(pm), _lib.ptr(nm), H, W, radius
        D.fx, D.fy, D.cx, D.cy = (float(v) for v in kk)
        D.robust_delta, D.w_sparse, D.w_dense = float(robust_delta), float(w_sparse), float(w_dense)
        D.dist_thresh, D.normal_thresh = float(dist_thresh), float(normal_thresh)
        D.depth_min, D.depth_max, D.min_trace = float(depth_min), float(depth_max), min_trace
        D.workspace, D.workspace_bytes = _lib.ptr(ws), ws.numel()
        D.poses_out, D.history = _lib.ptr(out), _lib.ptr(history)
        D.iter_poses, D.dbg_A, D.dbg_g, D.dbg_delta, D.dense_index = (_lib.ptr(dbg.get(k)) for k in (
            "iter_poses", "A", "g", "delta", "dense_index"))
        _lib.check(L.nof_pose_graph_optimize(ctypes.byref(D), _lib.stream_of(T)), what)
        # the workspace and inputs were used on the current stream only: the allocator may hand them on
    return (out, history, dbg) if return_debug else (out, history)
