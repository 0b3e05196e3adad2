"""Time pair_crops at the reference's shapes against the same crops written with torch ops.

10 frames of 640 x 480 (MeshRenderer renders of the sphere of the synthetic scene's mesh, vertex colours,
turned about the camera axis and tilted from frame to frame, with their masks) and all 45 pairs at S = 400:
90 crops. The torch route does the same work on the same GPU: the ROI by torch reductions over the masks,
one host read, pair_transforms on the host, then F.affine_grid / F.grid_sample (bilinear, zeros padding,
align_corners=True so that the sample coordinates are those of the kernel) over the masked float32 grey
frames, gathered per crop. Host clock around the whole call, its host read included, to a device synchronise;
medians of 3 after a warm-up. Kernel time alone, and the two kernels apart, are not measured. The largest
difference between the two routes' crops is recorded. Written to profiles/r23/pair_crops.json, not asserted.

    python scripts/pair_crops.py [--out-dir profiles/r23]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from scripts.transformer import _median_ms, _peak  # noqa: E402

H, W, S, N_FRAMES = 480, 640, 400, 10


def frames(dev):
    """-> (rgb [10,480,640,3] u8, masks [10,480,640] bool, poses [10,4,4] camera in world), device tensors and numpy."""
    from bundlesdf_amd.mesh import Mesh
    from bundlesdf_amd.mesh_render import MeshRenderer
    from tests import mesh_render_oracle as MR
    s = MR.scene()
    sphere = np.asarray(s["mesh"].faces)[s["ids"]["sphere"]]
    n = int(sphere.max()) + 1
    mesh = Mesh(np.asarray(s["mesh"].vertices)[:n].copy(), sphere.copy())
    mesh.vertex_colors = np.asarray(s["mesh"].vertex_colors)[:n].copy()
    mesh.vertex_normals = np.asarray(s["mesh"].vertex_normals)[:n].copy()
    K = np.array([[600.0, 0.0, 319.5], [0.0, 600.0, 239.5], [0.0, 0.0, 1.0]])
    ob_in_cam = np.stack([MR._pose([0.05 * f, -0.04 * f, 0.35 * f], [0.04 * f - 0.2, 0.02 * f - 0.1, 0.9 + 0.03 * f])
                          for f in range(N_FRAMES)])
    r = MeshRenderer(mesh, K, H, W, znear=MR.ZNEAR, zfar=MR.ZFAR, device=dev)
    out = r.render(ob_in_cam, colour="vertex")
    return out["rgb"].contiguous(), out["mask"].contiguous(), np.linalg.inv(ob_in_cam)


def torch_roi(masks):
    """[N,5] i32 (umin, umax, vmin, vmax, count) by torch reductions; an empty mask gives (W, -1, H, -1, 0)."""
    m = masks != 0
    N, h, w = m.shape
    cols, rows = m.any(1), m.any(2)
    u, v = torch.arange(w, device=m.device), torch.arange(h, device=m.device)
    umin = torch.where(cols, u, w).amin(1)
    umax = torch.where(cols, u, -1).amax(1)
    vmin = torch.where(rows, v, h).amin(1)
    vmax = torch.where(rows, v, -1).amax(1)
    return torch.stack([umin, umax, vmin, vmax, m.sum((1, 2))], 1).to(torch.int32)


def torch_pair_crops(P, rgb, masks, poses, pairs):
    host = torch_roi(masks).cpu().numpy()
    tf_a, tf_b, valid = P.pair_transforms(host, poses, pairs, H, W, S, 10)
    n = len(pairs)
    inv = P.invert_affine(np.stack([tf_a, tf_b], 1).reshape(2 * n, 3, 3))
    # crop pixel x = (xn + 1) (S - 1) / 2, source pixel sx = (sxn + 1) (W - 1) / 2: theta maps xn to sxn
    theta = np.empty((2 * n, 2, 3))
    half = (S - 1) / 2.0
    for i, size in ((0, W), (1, H)):
        theta[:, i, 0] = inv[:, i, 0] * half * 2.0 / (size - 1)
        theta[:, i, 1] = inv[:, i, 1] * half * 2.0 / (size - 1)
        theta[:, i, 2] = (inv[:, i, 0] * half + inv[:, i, 1] * half + inv[:, i, 2]) * 2.0 / (size - 1) - 1.0
    a = rgb.float()
    grey = ((0.2989 * a[..., 0] + 0.587 * a[..., 1]) + 0.114 * a[..., 2]) / 255.0
    grey = torch.where(masks != 0, grey, 0.0)
    idx = torch.from_numpy(np.asarray(pairs).reshape(-1)).to(rgb.device)
    grid = F.affine_grid(torch.from_numpy(theta).float().to(rgb.device), (2 * n, 1, S, S), align_corners=True)
    crops = F.grid_sample(grey[idx][:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
    return crops * torch.from_numpy(np.repeat(valid, 2)).to(rgb.device)[:, None, None]


def main():
    from bundlesdf_amd import pairs as P
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r23"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    os.makedirs(args.out_dir, exist_ok=True)
    rgb, masks, poses = frames(dev)
    pairs = np.array([(a, b) for a in range(N_FRAMES) for b in range(a + 1, N_FRAMES)])
    fused = lambda: P.pair_crops(rgb, masks, poses, pairs, out_size=S, margin=10)
    route = lambda: torch_pair_crops(P, rgb, masks, poses, pairs)
    res = dict(device=torch.cuda.get_device_name(0),
               timing="host clock around the whole call (ROI, its host read, the transforms on the host, the warp) to a "
                      "device synchronise, median of 3 after a warm-up; kernel time alone and the two kernels apart not "
                      "measured",
               frames=N_FRAMES, image=[H, W], pairs=len(pairs), crops=2 * len(pairs), out_size=S, source="uint8 RGB")
    res["pair_crops_ms"], res["pair_crops_ms_all"] = _median_ms(fused)
    res["torch_ms"], res["torch_ms_all"] = _median_ms(route)
    res["pair_crops_peak_bytes_allocated"] = _peak(fused)
    res["torch_peak_bytes_allocated"] = _peak(route)
    pc, ref = fused(), route()
    res["foreground_pixels_per_frame"] = pc.count.tolist()
    res["valid_pairs"] = int(pc.valid.sum())
    res["crop_mean"] = float(pc.images.mean())
    res["largest_difference_of_the_two_routes"] = float((pc.images - ref).abs().max())
    res["rms_difference_of_the_two_routes"] = float((pc.images - ref).square().mean().sqrt())
    res["cells_kept_fraction"] = float(pc.cells.float().mean())
    res["same_bytes_on_a_second_call"] = bool(torch.equal(fused().images, pc.images))
    with open(os.path.join(args.out_dir, "pair_crops.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("pair_crops_ms", "torch_ms", "largest_difference_of_the_two_routes",
                                          "valid_pairs", "crop_mean")}))


if __name__ == "__main__":
    main()
