#!/usr/bin/env python
"""Generate tests/golden/u_camera_paths.npz: the camera paths of the reference's data scripts, as data.

The reference modules are imported as they are -- scripts/data_utils.py (sample_on_sphere, get_camera_pose) and
utils/vis_utils.py (create_spheric_poses) -- with EMPTY stub modules for every import of theirs that this image does not have
(cv2, trimesh, pyrender, imageio, joblib, torchvision, plyfile ...: none of them is touched by the three functions called here),
the way gen_golden.py stubs kornia.  Only inputs and the reference's outputs are written; no reference source travels.
Re-run:  python tests/golden/gen_camera_paths.py   (needs /root/reference)"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


class _Stub(types.ModuleType):
    """An absent third-party module: a package whose every attribute is a placeholder."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def import_with_stubs(name):
    stubbed = []
    for _ in range(64):
        try:
            return importlib.import_module(name), stubbed
        except ModuleNotFoundError as e:
            if not e.name or e.name == name or e.name in sys.modules:
                raise
            sys.modules[e.name] = _Stub(e.name)
            stubbed.append(e.name)
    raise RuntimeError("too many missing modules: " + ", ".join(stubbed))


def main():
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "scripts"))
    data_utils, s1 = import_with_stubs("data_utils")
    vis_utils, s2 = import_with_stubs("utils.vis_utils")
    print("stubbed:", ", ".join(s1 + s2) or "nothing")
    out = {}
    # sample_on_sphere: (num, dist, half)
    sphere = [(120, 3.7416573867739413, False), (7, 1.0, False), (8, 2.5, True), (1, 1.0, False), (5, 0.5, True)]
    out["sphere_args"] = np.array([[n, d, h] for n, d, h in sphere], dtype=np.float64)
    for k, (n, d, h) in enumerate(sphere):
        out[f"sphere_{k}"] = np.asarray(data_utils.sample_on_sphere(n, d, h), dtype=np.float64)
    # get_camera_pose: positions from a spiral around a target, plus the two poles (the |z.z| >= 0.999 branch) and a near-pole
    target = np.array([0.1, -0.25, 3.5])
    pos = np.concatenate([out["sphere_1"] * 2.0 + target,
                          target + np.array([[0, 0, 2.0], [0, 0, -1.5], [0.01, 0.02, 1.0], [0.05, 0.0, 1.0]])])
    out["pose_target"] = target
    out["pose_positions"] = pos
    out["pose_out"] = np.stack([data_utils.get_camera_pose(p, target) for p in pos])
    # create_spheric_poses: (num, radius, center, vec_up or none)
    turn = [(30, 2.0, [0.0, 0.0, 0.0], None), (4, 3.5, [0.1, -0.2, 0.3], None), (6, 1.25, [0.0, 0.5, 0.0], [0.0, 1.0, 0.0]),
            (5, 2.0, [1.0, 2.0, 3.0], [0.2, -0.3, 0.9])]
    out["turn_args"] = np.array([[n, r] + c + (u if u is not None else [0.0, 0.0, 0.0]) + [u is not None] for n, r, c, u in turn],
                                dtype=np.float64)
    for k, (n, r, c, u) in enumerate(turn):
        res = vis_utils.create_spheric_poses(n, r, c, None if u is None else np.array(u))
        out[f"turn_{k}"] = np.asarray(res)
        assert out[f"turn_{k}"].dtype == np.float32
    path = os.path.join(HERE, "u_camera_paths.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
