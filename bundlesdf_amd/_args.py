"""Argument, device and weight plumbing shared by the Python wrappers.

What every wrapper needs before it can fill a descriptor of include/nof.h: an array or tensor as a
detached tensor or as a host array, the device a call runs on, a checkpoint's weights packed once
and kept per device, and the cell -> pixel rule of the two match classes. Nothing here launches a
kernel or validates a domain (shapes, ranges and their messages stay with the wrappers), and nothing
of the package is imported.
"""
import numpy as np
import torch

__all__ = ["as_tensor", "as_host", "default_device", "PackedWeights", "cells_to_pixels"]


def as_tensor(a, dtype=None):
    """a (array, list or tensor) -> a detached tensor on the device it came from. A tensor keeps its
    dtype; anything else is copied through numpy (as dtype, if given): the input may be read-only."""
    return a.detach() if torch.is_tensor(a) else torch.from_numpy(np.array(a, dtype=dtype))


def as_host(a, dtype=None):
    """a (array, list or tensor on any device) -> a C-contiguous numpy array of dtype (None: a's own),
    always a copy."""
    return np.array(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=dtype, order="C")


def default_device(t=None, device=None):
    """The device a call runs on: `device` if given, else t's if t is a tensor on the GPU, else the
    current HIP device. A HIP device always comes back with its index."""
    if device is not None:
        dev = torch.device(device)
    elif torch.is_tensor(t) and t.is_cuda:
        dev = t.device
    else:
        dev = torch.device("cuda")
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class PackedWeights:
    """Base of the classes that pack a checkpoint once into .packed (uint8, host) and keep one copy of it,
    and one byte buffer grown on demand, per device."""

    def __init__(self, packed, device=None):
        self.packed = packed
        self._weights = {}          # device -> uint8 tensor
        self._buffers = {}          # device -> uint8 tensor, grown on demand
        if device is not None:
            self.device_weights(device)

    @staticmethod
    def lookup(weights, prefix, key, shape, what):
        """weights[prefix + key] as a host array of its own dtype, refused unless it has `shape`."""
        if prefix + key not in weights:
            raise ValueError(f"{what}: key {prefix + key!r} is missing")
        v = as_host(weights[prefix + key])
        if tuple(v.shape) != shape:
            raise ValueError(f"{what}: key {prefix + key!r} has shape {tuple(v.shape)}, expected {shape}")
        return v

    @staticmethod
    def find_prefix(sd, probe, what, noun):
        """What stands before the key `probe` in the state dict sd, refused unless there is exactly one."""
        found = [k[:-len(probe)] for k in sd if k.endswith(probe)]
        if len(found) == 1:
            return found[0]
        if not found:
            raise ValueError(f"{what}: key {probe!r} is missing under every prefix")
        raise ValueError(f"{what}: prefixes {sorted(found)} all hold {noun}, name one")

    def device_weights(self, dev):
        """.packed on dev, copied there at the first call."""
        dev = default_device(device=dev)
        if dev not in self._weights:
            self._weights[dev] = torch.from_numpy(self.packed).to(dev)
        return self._weights[dev]

    def buffer(self, dev, nbytes):
        """dev's byte buffer, replaced by a larger one when it holds fewer than nbytes."""
        buf = self._buffers.get(dev)
        if buf is None or buf.numel() < nbytes:
            buf = self._buffers[dev] = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
        return buf


def cells_to_pixels(cell, w, pair, P, scale, tf, name, offset=None, rounded=True):
    """Cells [M] i64 of a grid of width w -> pixels [M,2] f64 on cell's device: (c % w, c // w) scale, plus
    offset [M,2] f64 in the descriptor image's frame, then through the inverse of tf ([3,3] or [P,3,3],
    row m by pair[m]), then rounded half away from zero unless rounded is False."""
    xy = torch.stack([cell % w, torch.div(cell, w, rounding_mode="floor")], 1).to(torch.float64) * float(scale)
    if offset is not None:
        xy = xy + offset
    if tf is not None:
        T = as_tensor(tf, np.float64).to(torch.float64).cpu()
        if tuple(T.shape) == (3, 3):
            T = T[None].expand(P, 3, 3)
        if tuple(T.shape) != (P, 3, 3):
            raise ValueError(f"to_pixels: {name} must be [3,3] or [{P},3,3], got {tuple(T.shape)}")
        Ti = torch.linalg.inv(T).to(cell.device)[pair]                  # [M,3,3]
        q = (Ti[:, :, 0] * xy[:, 0:1] + Ti[:, :, 1] * xy[:, 1:2]) + Ti[:, :, 2]
        xy = q[:, :2] / q[:, 2:3]
    # C round(): halves go away from zero, as lift_matches rounds its coordinates
    return torch.sign(xy) * torch.floor(torch.abs(xy) + 0.5) if rounded else xy
