#!/usr/bin/env python3
"""Generate tests/golden/m_mesh.npz: volumes and their isosurfaces from scikit-image's classic Lorensen-Cline marching cubes
(skimage.measure.marching_cubes(..., method="lorensen"), 0.18.3), the fixture set of the device marching cubes
(moco_flow_amd.mesh, tests/test_mesh_cpu.py, tests/test_gpu_mesh.py).

Two legs: this interpreter builds the volumes (numpy; the NeRF sigma lattice through oracle/cpu_ref.py, which needs torch),
then a second interpreter that has scikit-image meshes them (`--skimage-python`, default: this one).  Per fixture `<name>`
the file holds <name>_vol (float32), <name>_iso, <name>_clamp (max(v, 0) applied before meshing), <name>_verts (V, 3)
float32 and <name>_faces (T, 3) int32 as skimage returns them.  No value of a volume equals its isovalue.

usage:  python tests/golden/gen_mesh_golden.py [--skimage-python /path/to/python-with-skimage]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "m_mesh.npz")

NAMES = ("ball", "torus", "noise", "noncubic", "boundary", "nerf")
NERF_N = 28                 # sigma lattice side (visualize_mesh at N_grid = 28)
NERF_SIGMA_GAIN = 3.0       # sigma head of synth.nerf_state(0, regime="dense") x 3: its raw sigma then crosses 10


def grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def smooth_field(shape, seed, n_modes=24, max_freq=0.45):
    """Sum of random plane waves: a smooth field with many components of its isosurface."""
    rng = np.random.default_rng(seed)
    g = grid(shape)
    out = np.zeros(shape)
    for _ in range(n_modes):
        k = rng.uniform(-max_freq, max_freq, 3)
        out += rng.normal() * np.cos(k[0] * g[0] + k[1] * g[1] + k[2] * g[2] + rng.uniform(0, 2 * np.pi))
    return out


def nerf_sigma(N):
    """Raw sigma of visualize_mesh's lattice (np.linspace(-1.5, 1.5, N), np.meshgrid 'xy') through the oracle's NeRF."""
    import torch
    sys.path.insert(0, ROOT)
    from moco_flow_amd import synth
    from oracle import cpu_ref as R
    sd = synth.nerf_state(0, regime="dense")
    sd["sigma.weight"] = sd["sigma.weight"] * np.float32(NERF_SIGMA_GAIN)
    x = np.linspace(-1.5, 1.5, N)
    xyz = torch.FloatTensor(np.stack(np.meshgrid(x, x, x), -1).reshape(-1, 3))
    with torch.no_grad():
        s = R.build_nerf(sd)(R._embed_padded(R.Embedding(3, 10), xyz, 63), sigma_only=True)
    return s.numpy().reshape(N, N, N)


def volumes():
    vols = {}
    g = grid((24, 24, 24))
    vols["ball"] = (np.sqrt((g[0] - 10.3) ** 2 + (g[1] - 12.7) ** 2 + (g[2] - 11.1) ** 2) - 7.45, 0.0, False)
    g = grid((32, 32, 32))
    rho = np.sqrt((g[0] - 15.6) ** 2 + (g[1] - 16.2) ** 2)
    vols["torus"] = (np.sqrt((rho - 9.1) ** 2 + (g[2] - 15.3) ** 2) - 3.7, 0.0, False)
    vols["noise"] = (smooth_field((20, 20, 20), 1), 0.1, False)
    vols["noncubic"] = (smooth_field((17, 23, 31), 2), -0.2, False)
    g = grid((16, 18, 20))
    vols["boundary"] = (np.sqrt((g[0] - 1.2) ** 2 + (g[1] - 9.4) ** 2 + (g[2] - 18.6) ** 2) - 6.3, 0.0, False)
    vols["nerf"] = (nerf_sigma(NERF_N), 10.0, True)
    out = {}
    for name, (v, iso, clamp) in vols.items():
        v = v.astype(np.float32)
        assert not np.any((np.maximum(v, 0) if clamp else v) == np.float32(iso)), name
        out[name + "_vol"], out[name + "_iso"], out[name + "_clamp"] = v, np.float32(iso), np.bool_(clamp)
    return out


def mesh_leg(inp, outp):
    from skimage.measure import marching_cubes
    d = dict(np.load(inp))
    for name in NAMES:
        v = d[name + "_vol"]
        if d[name + "_clamp"]:
            v = np.maximum(v, 0)
        verts, faces, _, _ = marching_cubes(v, float(d[name + "_iso"]), method="lorensen")
        d[name + "_verts"], d[name + "_faces"] = verts.astype(np.float32), faces.astype(np.int32)
    np.savez_compressed(outp, **d)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--mesh-leg":
        return mesh_leg(sys.argv[2], sys.argv[3])
    py = sys.argv[sys.argv.index("--skimage-python") + 1] if "--skimage-python" in sys.argv else sys.executable
    with tempfile.TemporaryDirectory() as tmp:
        inp = os.path.join(tmp, "vols.npz")
        np.savez(inp, **volumes())
        subprocess.run([py, "-W", "ignore", os.path.abspath(__file__), "--mesh-leg", inp, OUT], check=True)
    d = np.load(OUT)
    for name in NAMES:
        print(f"{name:9s} {str(d[name + '_vol'].shape):14s} iso {float(d[name + '_iso']):5.1f}: "
              f"V {len(d[name + '_verts']):6d}  T {len(d[name + '_faces']):6d}")


if __name__ == "__main__":
    main()
