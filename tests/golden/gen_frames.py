"""Writes tests/golden/u_frames.npz: seeded inputs, PIL's own outputs for the resize cases and the reference's float64 plate
expression (scripts/data_utils.py:150-163, through tests/frames_oracle.py::plate_float64) for the plate cases.

    python tests/golden/gen_frames.py            (needs PIL; the tests read only the .npz)

PIL is the library the reference calls (T.Resize on a PIL image, datasets/moco_flow_dataset.py:51-55): its outputs are recorded
data.  Keys: `cases` (JSON: the case tables below), `in_<name>` inputs, `resize_<case>` PIL's outputs, `plate_<case>_frames`,
`_masks`, `_f64`."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

ALPHAS = (0, 1, 3, 128, 254, 255)

# input name -> (F, H0, W0, C)
INPUTS = {
    "a4": (3, 37, 53, 4), "a3": (1, 37, 53, 3), "a1": (1, 37, 53, 1),
    "b4": (1, 23, 19, 4), "b3": (1, 23, 20, 3),
    "tall3": (1, 300, 3, 3), "wide4": (1, 3, 300, 4),
    "dot4": (1, 1, 1, 4), "dot1": (1, 1, 1, 1), "s3": (1, 5, 6, 3), "s4": (2, 5, 6, 4),
    "h4": (1, 64, 48, 4),
}
# case name -> (input, H, W)
RESIZE_CASES = {
    "down_rgba_f3": ("a4", 16, 20), "down_rgb": ("a3", 16, 20), "down_l": ("a1", 16, 20),
    "share_exact": ("a4", 16, 16), "share_minus": ("a4", 15, 17), "share_plus": ("a4", 1, 257),
    "up_rgba": ("b4", 40, 31), "up_rgb": ("b3", 40, 31),
    "taps87_v": ("tall3", 7, 3), "taps87_h": ("wide4", 3, 7),
    "dot_up_rgba": ("dot4", 5, 4), "dot_up_l": ("dot1", 5, 4), "to_dot_rgb": ("s3", 1, 1), "to_dot_rgba": ("s4", 1, 1),
    "h_only_rgba": ("a4", 37, 20), "v_only_rgba": ("a4", 16, 53), "h_only_rgb": ("a3", 37, 20), "v_only_rgb_bytes": ("a3", 16, 53),
    "v_only_rgb_words": ("b3", 9, 20), "h_only_l": ("a1", 37, 21), "v_only_l": ("a1", 9, 53),
    "half_rgba": ("h4", 32, 24), "identity_rgba": ("a4", 37, 53),
}
# case name -> (F, H, W, C, k, soft masks)
PLATE_CASES = {
    "f1": (1, 8, 8, 4, 0, False), "f2": (2, 8, 8, 3, 1, True), "f5": (5, 8, 8, 4, 4, True),
    "f64": (64, 8, 8, 4, 51, False), "f65": (65, 8, 8, 3, 52, True), "f300": (300, 3, 5, 4, 240, True),
}


def make_input(rng, F, H, W, C):
    a = rng.integers(0, 256, size=(F, H, W, C), dtype=np.uint8)
    if C == 4:
        fixed = rng.choice(np.array(ALPHAS, dtype=np.uint8), size=(F, H, W))
        a[..., 3] = np.where(rng.random((F, H, W)) < 0.6, fixed, a[..., 3])
    return a


def pil_resize(a, H, W):
    from PIL import Image
    out = []
    for fr in a:
        im = Image.fromarray(fr[..., 0] if fr.shape[2] == 1 else fr)
        r = np.asarray(im.resize((W, H), Image.BILINEAR))
        out.append(r[..., None] if fr.shape[2] == 1 else r)
    return np.stack(out)


def main():
    import PIL
    import frames_oracle as FO
    rng = np.random.default_rng(20240607)
    data = {"cases": np.array(json.dumps({"inputs": INPUTS, "resize": RESIZE_CASES, "plate": PLATE_CASES, "pil": PIL.__version__}))}
    inputs = {name: make_input(rng, *shape) for name, shape in INPUTS.items()}
    for name, a in inputs.items():
        data["in_" + name] = a
    for case, (src, H, W) in RESIZE_CASES.items():
        data["resize_" + case] = pil_resize(inputs[src], H, W)
    for case, (F, H, W, C, k, soft) in PLATE_CASES.items():
        frames, masks = FO.plate_inputs(rng, F, H, W, C, soft)
        data[f"plate_{case}_frames"], data[f"plate_{case}_masks"] = frames, masks
        data[f"plate_{case}_f64"] = FO.plate_float64(frames, masks, k)
    path = os.path.join(HERE, "u_frames.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
