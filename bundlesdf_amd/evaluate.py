"""Pose and mesh evaluation on the device: ADD, ADD-S, their AUC, chamfer distance.

The scoring of a finished run, as the reference's HO3D benchmark does it
(benchmark_ho3d.py:18-139 with Utils.py:82-103,175-198,268-273): ADD / ADD-S
per frame and their AUC for the pose track, and for the mesh a clean-up, the
largest component, a surface sample, a point-to-point ICP to the ground-truth
cloud and the mutual chamfer distance. The reference builds a cKDTree per
frame (ADD-S), two for the chamfer distance and lets open3d search once per ICP
iteration; here every one of those searches is nof_nearest_points
(csrc/nearest.hip), an exact nearest-neighbour search in a uniform cell grid,
and the ICP's sums are nof_correspondence_moments.

No CPU fallback: everything that searches raises if libnof.so cannot run.
compute_auc and the first-frame alignment are host numpy, as in the reference.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._args import as_host, as_tensor, default_device
from .handoff import PointCloud
from .mesh import trimesh_clean, trimesh_split

__all__ = ["PointGrid", "nearest", "add_err", "adi_err", "compute_auc", "chamfer_distance_between_clouds_mutual",
           "sample_surface", "icp_point_to_point", "correspondence_moments", "align_first_frame", "evaluate_poses",
           "evaluate_mesh", "mesh_frame_agreement"]

MAX_GRID_CELLS = 1 << 24
RIGID_TOL = 1e-6          # max |R R^T - I| of a pose add_err / adi_err accept
_FRAME_CHUNK_POINTS = 1 << 22   # add_err: frames x model points transformed at a time


def _points(a, device):
    return as_tensor(a, np.float64).to(device, torch.float64).reshape(-1, 3).contiguous()


class PointGrid:
    """A point cloud [N,3] held in a uniform cell grid on the device (nof_point_grid_build with
    cell_ids), the search structure of `nearest`.

    cell: the cell edge. Default 2 * (bbox volume / N) ** (1/3), about eight points per cell of a
    cloud that fills its box. An axis of zero extent gets one cell and is left out of that volume
    (a planar cloud takes the square root of area / N); a cloud of one position gets one cell.
    The edge grows by a quarter at a time until the grid has at most 2^24 cells."""

    def __init__(self, points, cell=None, device=None):
        self.device = default_device(points, device)
        p = _points(points, self.device)
        n = len(p)
        if n == 0:
            raise ValueError("PointGrid: empty point cloud")
        if not bool(torch.isfinite(p).all()):
            raise ValueError("PointGrid: non-finite point")
        lo, hi = p.min(0).values.cpu().numpy(), p.max(0).values.cpu().numpy()
        ext = hi - lo
        if cell is None:
            nz = ext[ext > 0]
            cell = 2.0 * float(np.prod(nz) / n) ** (1.0 / len(nz)) if len(nz) else 1.0
        cell = float(cell)
        if not cell > 0:
            raise ValueError(f"PointGrid: cell must be > 0, got {cell}")
        while True:
            dims = np.where(ext > 0, np.floor(ext / cell) + 1, 1.0)     # f64: the product cannot overflow
            if float(np.prod(dims)) <= MAX_GRID_CELLS:
                break
            cell *= 1.25
        self.points, self.n, self.cell = p, n, cell
        self.origin = lo.astype(np.float64)
        self.dims = dims.astype(np.int32)
        nc = int(np.prod(dims))
        L = _lib.lib()
        with torch.cuda.device(self.device):
            self.cell_start = torch.empty(nc + 1, dtype=torch.int32, device=self.device)
            self.cell_points = torch.empty_like(p)
            self.cell_ids = torch.empty(n, dtype=torch.int32, device=self.device)
            ws = torch.empty(int(L.nof_point_grid_workspace_bytes(nc)), dtype=torch.uint8, device=self.device)
            self._origin_c = (ctypes.c_double * 3)(*self.origin.tolist())
            self._dims_c = (ctypes.c_int32 * 3)(*self.dims.tolist())
            _lib.check(L.nof_point_grid_build(_lib.ptr(p), n, self._origin_c, self._dims_c, ctypes.c_double(cell),
                                              _lib.ptr(self.cell_start), _lib.ptr(self.cell_points),
                                              _lib.ptr(self.cell_ids), _lib.ptr(ws), _lib.stream_of(p)),
                       "point_grid_build")
        self._keep = ws

    def __len__(self):
        return self.n


def _as_grid(cloud_or_grid, device=None):
    return cloud_or_grid if isinstance(cloud_or_grid, PointGrid) else PointGrid(cloud_or_grid, device=device)


def nearest(queries, cloud_or_grid, transforms=None, max_dist=None):
    """Exact nearest neighbour of every query in a cloud -> (dist, index), device tensors (f64, int32).

    queries [Q,3]; cloud_or_grid a PointGrid or points [N,3] (a grid is built). transforms: None or
    one 4x4 -> results [Q]; [B,4,4] -> [B,Q], query q searched at T_b q. index is the lowest index of
    the cloud among its closest points (d2 = (dx dx + dy dy) + dz dz in f64), dist = sqrt(d2). With
    max_dist, a query whose distance is above it gets index -1 and dist inf."""
    grid = _as_grid(cloud_or_grid, queries.device if torch.is_tensor(queries) and queries.is_cuda else None)
    dev = grid.device
    q = _points(queries, dev)
    Q = len(q)
    T, single = None, True
    if transforms is not None:
        T = as_tensor(transforms, np.float64)
        single = T.dim() == 2
        T = T.to(dev, torch.float64).reshape(-1, 4, 4).contiguous()
    B = 1 if T is None else len(T)
    md = 0.0 if max_dist is None else float(max_dist)
    if max_dist is not None and not md > 0:
        raise ValueError(f"nearest: max_dist must be > 0, got {max_dist}")
    index = torch.empty((B, Q), dtype=torch.int32, device=dev)
    dist = torch.empty((B, Q), dtype=torch.float64, device=dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        for b0 in range(0, B, 65535):   # the entry point takes up to 65535 transforms a launch
            nb = min(65535, B - b0)
            _lib.check(L.nof_nearest_points(_lib.ptr(q), Q, _lib.ptr(T[b0:b0 + nb]) if T is not None else None, nb,
                                            _lib.ptr(grid.cell_start), _lib.ptr(grid.cell_points),
                                            _lib.ptr(grid.cell_ids), grid.n, grid._origin_c, grid._dims_c,
                                            ctypes.c_double(grid.cell), ctypes.c_double(md), _lib.ptr(index[b0:]),
                                            _lib.ptr(dist[b0:]), _lib.stream_of(q)), "nearest_points")
    return (dist[0], index[0]) if single else (dist, index)


def _poses(pred, gt, what):
    """(pred [F,4,4], gt [F,4,4], single) as host f64; every rotation block must be orthonormal."""
    P, G = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    single = P.ndim == 2
    P, G = P.reshape(-1, 4, 4), G.reshape(-1, 4, 4)
    if len(P) != len(G):
        raise ValueError(f"{what}: {len(P)} predicted poses, {len(G)} ground-truth poses")
    for name, A in (("pred", P), ("gt", G)):
        if len(A) == 0:
            continue
        R = A[:, :3, :3]
        err = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).reshape(len(A), -1).max(1)
        if not np.all(err <= RIGID_TOL):     # also catches NaN
            f = int(np.argmax(~(err <= RIGID_TOL)))
            raise ValueError(f"{what}: {name} pose {f} is not rigid (max |R R^T - I| = {err[f]:.3g} > {RIGID_TOL})")
    return P, G, single


def add_err(pred, gt, model_pts):
    """ADD (Hinterstoisser et al., ACCV 2012; Utils.py:82-90): mean distance between the model points
    under the predicted and the ground-truth pose. One 4x4 each -> float; [F,4,4] -> [F] f64 numpy.
    Poses must be rigid (ValueError otherwise)."""
    P, G, single = _poses(pred, gt, "add_err")
    dev = default_device(model_pts)
    m = _points(model_pts, dev)
    Pd, Gd = torch.from_numpy(P).to(dev), torch.from_numpy(G).to(dev)
    out = torch.empty(len(P), dtype=torch.float64, device=dev)
    step = max(1, _FRAME_CHUNK_POINTS // max(1, len(m)))
    for f0 in range(0, len(P), step):
        a = m @ Pd[f0:f0 + step, :3, :3].transpose(1, 2) + Pd[f0:f0 + step, None, :3, 3]
        b = m @ Gd[f0:f0 + step, :3, :3].transpose(1, 2) + Gd[f0:f0 + step, None, :3, 3]
        out[f0:f0 + step] = (a - b).norm(dim=2).mean(1)
    e = out.cpu().numpy()
    return float(e[0]) if single else e


def adi_err(pred, gt, model_pts):
    """ADD-S (Utils.py:92-103): mean distance from each model point under the ground-truth pose to the
    closest model point under the predicted pose. One 4x4 each -> float; [F,4,4] -> [F] f64 numpy.

    One grid is built over model_pts and the model points moved by inv(pred_f) @ gt_f are searched in
    it, every frame in one launch. For rigid poses |gt m - pred m'| = |inv(pred) gt m - m'|, so this is
    the reference's distance up to the rounding of the transforms; a pose whose rotation block is not
    orthonormal to 1e-6 would give another number and raises ValueError instead. `model_pts` may be a
    PointGrid, to score several tracks against one model."""
    P, G, single = _poses(pred, gt, "adi_err")
    grid = _as_grid(model_pts)
    if len(P) == 0:
        return np.zeros(0)
    rel = np.linalg.inv(P) @ G
    dist, _ = nearest(grid.points, grid, transforms=rel)
    e = dist.mean(1).cpu().numpy()
    return float(e[0]) if single else e


def compute_auc(errs, max_val=0.1):
    """Area under the accuracy-threshold curve up to max_val, as a fraction of max_val (Utils.py:175-198,
    the YCB-Video protocol): the step curve that rises by 1/n at each sorted error, integrated from 0 to
    max_val with each step's height taken at its right end.

    Empty input returns 0. When no error is below max_val the result is 0.0; the reference indexes an
    empty array there (prec[-1]) and raises IndexError."""
    e = np.sort(np.asarray(errs, np.float64).reshape(-1))
    n = len(e)
    if n == 0:
        return 0
    k = int(np.searchsorted(e, max_val, side="left"))     # errors strictly below max_val
    if k == 0:
        return 0.0
    x = np.concatenate([[0.0], e[:k], [max_val]])
    y = np.concatenate([np.arange(1, k + 1) / float(n), [k / float(n)]])
    return float(np.sum(np.diff(x) * y) / max_val)


def chamfer_distance_between_clouds_mutual(pts1, pts2):
    """Utils.py:268-273: 0.5 * (mean NN distance of pts2 in pts1 + mean NN distance of pts1 in pts2)."""
    g1 = _as_grid(pts1)
    g2 = _as_grid(pts2, g1.device)
    d1, _ = nearest(g2.points, g1)
    d2, _ = nearest(g1.points, g2)
    return 0.5 * (float(d1.mean()) + float(d2.mean()))


def sample_surface(mesh, count, seed=0, device=None):
    """`count` points on a mesh's surface -> (points [count,3] f64, face_index [count] i64), device tensors.

    As trimesh.sample.sample_surface(mesh, count): faces chosen with probability proportional to their
    area, points uniform in the face (barycentric, the pair reflected when it falls outside). The draws
    come from a torch.Generator on the device seeded with `seed`: the same seed gives the same points,
    but trimesh's numpy stream cannot be reproduced here — only the distribution matches."""
    dev = default_device(device=device)
    v = torch.from_numpy(np.ascontiguousarray(mesh.vertices, np.float64)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(mesh.faces, np.int64)).to(dev)
    if len(f) == 0:
        raise ValueError("sample_surface: mesh has no faces")
    tri = v[f]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    cum = torch.cumsum(0.5 * torch.linalg.cross(e1, e2).norm(dim=1), 0)
    if not float(cum[-1]) > 0:
        raise ValueError("sample_surface: mesh has no area")
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    r = torch.rand((int(count), 3), dtype=torch.float64, device=dev, generator=gen)
    face = torch.searchsorted(cum, r[:, 0] * cum[-1], right=True).clamp_(max=len(f) - 1)
    u, w = r[:, 1], r[:, 2]
    flip = u + w > 1.0
    u, w = torch.where(flip, 1.0 - u, u), torch.where(flip, 1.0 - w, w)
    pts = tri[face, 0] + u[:, None] * e1[face] + w[:, None] * e2[face]
    return pts, face


def correspondence_moments(source, target, index, dist, transform=None):
    """The 17 sums of nof_correspondence_moments over the pairs with index >= 0, as host f64: count,
    sum p' (3), sum q (3), sum p' q^T (9), sum dist^2, with p' = transform applied to source and
    q = target[index]. source / target / index / dist are device tensors."""
    dev = source.device
    n, m = len(source), len(target)
    L = _lib.lib()
    T = None if transform is None else torch.as_tensor(np.asarray(transform, np.float64)).to(dev).contiguous()
    with torch.cuda.device(dev):
        sums = torch.empty(17, dtype=torch.float64, device=dev)
        ws = torch.empty(max(1, int(L.nof_nearest_workspace_bytes(n))), dtype=torch.uint8, device=dev)
        _lib.check(L.nof_correspondence_moments(_lib.ptr(source), n, _lib.ptr(T), _lib.ptr(target), m,
                                                _lib.ptr(index), _lib.ptr(dist), _lib.ptr(sums), _lib.ptr(ws),
                                                _lib.stream_of(source)), "correspondence_moments")
    return sums.cpu().numpy()


def _kabsch(s):
    """Rigid update (no scale, reflection corrected) from the 17 sums: the 4x4 that best moves the
    p' onto their q in the least-squares sense."""
    n = s[0]
    pm, qm = s[1:4] / n, s[4:7] / n
    H = s[7:16].reshape(3, 3) / n - np.outer(pm, qm)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, qm - R @ pm
    return T


def icp_point_to_point(source, target, max_dist, init=np.eye(4), max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
    """Point-to-point ICP of `source` onto `target` (points [N,3] or a PointGrid) -> dict with
    transformation [4,4], fitness (share of source points with a target point within max_dist),
    inlier_rmse and iterations.

    Per iteration: `nearest` with max_dist of the source moved by the current transform, the 17 sums
    (nof_correspondence_moments), a 3x3 Kabsch update from them on the host in f64 composed on the
    left. It stops when fitness and inlier_rmse both change by less than rel_fitness / rel_rmse, when
    there are no correspondences, or after max_iter updates. The loop and the defaults (30, 1e-6, 1e-6)
    are open3d's documented registration_icp with TransformationEstimationPointToPoint, which the
    reference calls; open3d is not available to this project's tests, so parity with it is unpinned."""
    grid = _as_grid(target)
    src = _points(source, grid.device)
    T = np.array(init, np.float64).reshape(4, 4)
    n = len(src)

    def score(T):
        dist, index = nearest(src, grid, transforms=T, max_dist=max_dist)
        s = correspondence_moments(src, grid.points, index, dist, T)
        return s, (s[0] / n if n else 0.0), (float(np.sqrt(s[16] / s[0])) if s[0] > 0 else 0.0)

    s, fitness, rmse = score(T)
    it = 0
    while it < max_iter and s[0] > 0:
        T = _kabsch(s) @ T
        it += 1
        prev = (fitness, rmse)
        s, fitness, rmse = score(T)
        if abs(prev[0] - fitness) < rel_fitness and abs(prev[1] - rmse) < rel_rmse:
            break
    return {"transformation": T, "fitness": float(fitness), "inlier_rmse": float(rmse), "iterations": it}


def align_first_frame(pred_poses, gt_poses):
    """benchmark_ho3d.py:60-62: the predicted track moved so that its first pose is the first
    ground-truth pose, pred @ inv(pred[0]) @ gt[0] (host f64)."""
    P, G = np.asarray(pred_poses, np.float64).reshape(-1, 4, 4), np.asarray(gt_poses, np.float64).reshape(-1, 4, 4)
    if len(P) == 0:
        return P.copy()
    return P @ np.linalg.inv(P[0]) @ G[0]


def evaluate_poses(pred_poses, gt_poses, model_pts):
    """The benchmark's pose leg (benchmark_ho3d.py:60-78): first-frame alignment, then per frame ADD and
    ADD-S over model_pts -> {"ADD": [F] m, "ADDS": [F] m, "ADD_AUC": %, "ADDS_AUC": %}."""
    P = align_first_frame(pred_poses, gt_poses)
    G = np.asarray(gt_poses, np.float64).reshape(-1, 4, 4)
    grid = _as_grid(model_pts)
    adds = adi_err(P, G, grid)
    add = add_err(P, G, grid.points)
    return {"ADD": add, "ADDS": adds, "ADD_AUC": compute_auc(add) * 100, "ADDS_AUC": compute_auc(adds) * 100}


def _clean(mesh):
    """Utils.py:278-284: mesh.trimesh_clean (weld, degenerate and duplicate faces, unused vertices)."""
    return trimesh_clean(mesh)


def evaluate_mesh(pred_mesh, gt_pts, voxel=0.005, n_samples=99999, icp_thres=0.02, min_edge=1000, seed=0,
                  backend="hip"):
    """The benchmark's mesh leg (benchmark_ho3d.py:93-128) for a predicted mesh already in the frame of
    gt_pts [M,3] (metres) -> {"chamfer_cm", "icp", "component"}.

    Vertices outside gt_pts' box grown by 0.3 m are dropped; the mesh is cleaned (merge_vertices,
    degenerate and duplicate faces, unreferenced vertices); trimesh_split(min_edge, backend), again with
    min_edge=3 when that leaves nothing; of the components with a vertex within 0.1 m of the origin the
    one with the most vertices is kept. n_samples surface points of it (sample_surface, seed), voxel
    down-sampled, are registered to gt_pts by icp_point_to_point(icp_thres); all samples moved by the
    result give the mutual chamfer distance to gt_pts, in cm. The input mesh is not modified."""
    if backend not in ("scipy", "hip"):
        raise ValueError(f"evaluate_mesh: backend must be 'scipy' or 'hip', got {backend!r}")
    gt = as_host(gt_pts, np.float64).reshape(-1, 3)
    mesh = pred_mesh.copy()
    hi, lo = gt.max(0) + 0.3, gt.min(0) - 0.3
    mesh.update_vertices(~((mesh.vertices > hi).any(1) | (mesh.vertices < lo).any(1)))
    _clean(mesh)
    parts = trimesh_split(mesh, min_edge=min_edge, backend=backend)
    if not parts:
        parts = trimesh_split(mesh, min_edge=3, backend=backend)
    best = None
    for part in parts:
        if np.linalg.norm(part.vertices, axis=1).min() > 0.1:
            continue
        if best is None or len(part.vertices) > len(best.vertices):
            best = part
    if best is None:
        raise ValueError("evaluate_mesh: no mesh component within 0.1 m of the origin")
    gt_grid = PointGrid(gt)
    pts, _ = sample_surface(best, n_samples, seed=seed, device=gt_grid.device)
    down = PointCloud(pts, device=gt_grid.device).voxel_down_sample(voxel)
    icp = icp_point_to_point(down._p, gt_grid, icp_thres)
    T = torch.from_numpy(icp["transformation"]).to(gt_grid.device)
    moved = (pts @ T[:3, :3].T + T[:3, 3]).contiguous()
    cd = chamfer_distance_between_clouds_mutual(moved, gt_grid) * 100
    return {"chamfer_cm": cd, "icp": icp, "component": best}


def mesh_frame_agreement(render_depth, render_mask, obs_depth, obs_mask, max_depth):
    """How well a rendered mesh (MeshRenderer.render's depth and mask) coincides with observed frames,
    per frame: [H,W] or [F,H,W] arrays or tensors on any device -> {"iou", "depth_mean", "depth_median"
    (float64 [F]) and "count" (int64 [F])}, tensors on the inputs' device.

    A rendered pixel is valid where its mask is set and 0 < depth <= max_depth; an observed one
    likewise (the frames' 0 and their far fill both fall out). iou is the intersection of the two
    valid sets over their union; depth_mean / depth_median are the mean and the median (the lower of
    the two middle values for an even count) of |rendered - observed| over the intersection, count
    is its size. A frame with an empty intersection reports iou 0 (also when the union is empty),
    count 0 and differences 0: no NaN."""
    rd, rm, od, om = (as_tensor(a) for a in (render_depth, render_mask, obs_depth, obs_mask))
    dev = rd.device
    H, W = rd.shape[-2:]
    rd, od = rd.reshape(-1, H * W).double(), od.to(dev).reshape(-1, H * W).double()
    rm, om = rm.to(dev).reshape(-1, H * W) != 0, om.to(dev).reshape(-1, H * W) != 0
    if not (rd.shape == od.shape == rm.shape == om.shape):
        raise ValueError("mesh_frame_agreement: the four images must have one shape")
    a = rm & (rd > 0) & (rd <= max_depth)
    b = om & (od > 0) & (od <= max_depth)
    both = a & b
    count = both.sum(1)
    union = (a | b).sum(1)
    iou = torch.where(union > 0, count.double() / union.clamp(min=1).double(), torch.zeros_like(count, dtype=torch.float64))
    diff = torch.where(both, (rd - od).abs(), torch.full_like(rd, float("inf")))
    mean = torch.where(both, diff, torch.zeros_like(diff)).sum(1) / count.clamp(min=1).double()
    srt = torch.sort(diff, dim=1).values                       # the intersection's differences first
    mid = ((count - 1).clamp(min=0) // 2)[:, None]
    median = torch.where(count > 0, srt.gather(1, mid)[:, 0], torch.zeros_like(mean))
    return {"iou": iou, "depth_mean": mean, "depth_median": median, "count": count}
