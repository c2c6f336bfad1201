"""Shared builders: turn a golden render case into (rays, bg, embeddings, models, kwargs)
for either backend -- ``oracle.cpu_ref`` (CPU checker) or ``moco_flow_amd`` (HIP product)."""
import os

import numpy as np
import torch

from cases import RENDER_CASES  # tests/golden/cases.py
from moco_flow_amd import synth

TOL = 1e-4      # max-rel of the fp32 contract (tests/test_gpu_parity.py)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def relerr(a, b):
    """max|a-b| / max|b|  (SURVEY.md §8d 'max-rel')."""
    a = torch.as_tensor(a).detach().to(torch.float64).cpu()
    b = torch.as_tensor(b).detach().to(torch.float64).cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    if b.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def pdf_per_wave_floats(nb, Mi):
    """The LDS floats one ray's wave needs in mf_sample_pdf, as its entry point computes them (four 16-byte aligned arrays:
    the S + M depths, bins, cdf, pdf); a workgroup is four waves and the limit 64 KiB."""
    r4 = lambda n: (n + 3) & ~3
    return r4(nb + 1 + Mi) + 2 * r4(nb) + r4(nb - 1)


def _l2rel(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def build_case(backend, case, seed, device="cpu", tags=None):
    """backend: a module exposing Embedding / NeRF / NoF classes with the reference's
    constructor signatures and ``load_state_dict``."""
    c = case if isinstance(case, dict) else RENDER_CASES[case]
    tags = tags or {}          # weight-stream names per role (bench.py draws "nerf" / "nerf_fine" / "bw" / "fw")
    nof = c.get("nof", "none")
    extra = c["extra"]
    extra_dim = {"dir": 27, "ind": 5, "none": 0}[extra]

    def emb(cin, nf, weights=None):
        e = backend.Embedding(cin, nf, True)
        if weights is not None:
            e.weights = list(weights)
        return e

    def nerf(tag):
        m = backend.NeRF(8, 256, 63, [4], extra, extra_dim)
        sd = synth.nerf_state(seed, extra_feat_type=extra, extra_feat_dim=extra_dim,
                              regime=c["regime"], tag=tags.get(tag, tag))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return m.to(device) if hasattr(m, "to") else m

    def nof_model(tag):
        m = backend.NoF(4, 128, 33, [2], "ind", 33, c.get("quat", True))
        sd = synth.nof_state(seed, use_quat=c.get("quat", True), tag=tags.get(tag, tag), head_scale=0.25)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        return m.to(device) if hasattr(m, "to") else m

    nerf_embs = [emb(3, c.get("xyz_freqs", 10), c.get("xyz_w")),
                 emb(1, 2) if extra == "ind" else None,
                 emb(3, 4) if extra == "dir" else None]
    nerfs = [nerf("coarse")] + ([nerf("fine")] if c["M"] > 0 else [])
    nof_embs = nof_models = None
    if nof != "none":
        nof_embs = [emb(3, 5), emb(1, 16)]
        nof_models = [nof_model("bw")] + ([nof_model("fw")] if nof in ("local", "global") else [])
    kw = dict(nof_embeddings=nof_embs, nof_models=nof_models,
              chain_local=nof in ("local", "global"), chain_global=nof == "global",
              N_samples=c["S"], N_importance=c["M"], use_disp=c.get("disp", False), perturb=0,
              noise_std=0, nerf_activate_type=c.get("act", "relu"), test_time=c.get("test", False))
    return nerf_embs, nerfs, kw


def case_inputs(c, seed, n=None, device="cpu"):
    nof = c.get("nof", "none")
    n = c["n"] if n is None else n
    rays, bg = synth.rays(seed, n, chained=(nof == "global"))
    rays = torch.from_numpy(rays).to(device)
    bg = torch.from_numpy(bg).to(device) if c.get("bg", True) else None
    return rays, bg


def varied_indices(rays, seed=0):
    """``rays`` with per-ray image indices: columns 8 (and 9 when present) become seeded permutations of
    linspace(-1, 1) over the batch (values in [-1, 1)), so that neighbouring rays differ -- synth.rays gives every ray one
    index, under which a kernel that stages another ray's index bias row renders the same numbers."""
    rays = rays.clone()
    n = rays.shape[0]
    grid = torch.linspace(-1.0, 1.0, n + 1, dtype=torch.float64)[:n].to(rays.dtype)
    gen = torch.Generator().manual_seed(seed)
    for col in range(8, min(rays.shape[1], 10)):
        rays[:, col] = grid[torch.randperm(n, generator=gen)].to(rays.device)
    return rays


def subset_rays(n, k, seed=0):
    """Sorted indices of at most k of n rays: the first and the last k / 8 (at least 4, at most 32), the rest a seeded draw
    from between them.  Per-ray outputs do not depend on the other rays of a batch (tests/test_oracle_golden.py), so an
    oracle of rays[idx] checks a kernel's launch over all n rays at these."""
    if n <= k:
        return torch.arange(n)
    e = max(4, min(32, k // 8))
    mid = torch.randperm(n - 2 * e, generator=torch.Generator().manual_seed(seed))[:k - 2 * e] + e
    return torch.cat([torch.arange(e), mid.sort().values, torch.arange(n - e, n)])


class OracleOps:
    """CPU stand-ins, backed by oracle.cpu_ref, for the building blocks the backward unit tests differentiate: the same
    weights as a product module in an oracle container whose tensors are autograd leaves (``twin``), and the oracle's
    embedding / network / chain / composite functions on CPU copies of the inputs.  (Round 2 compared the HIP nodes with
    an eager restatement that lived inside the package; the checker is the oracle.)"""

    def __init__(self, R):
        self.R = R
        self.twins = {}

    def twin(self, m):
        if id(m) not in self.twins:
            sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
            if hasattr(m, "use_quat"):
                t = self.R.NoF(m.D, m.W, m.in_channels_xyz, list(m.skips), m.extra_feat_type, m.extra_feat_dim, m.use_quat, state=sd)
            else:
                t = self.R.NeRF(m.D, m.W, m.in_channels_xyz, list(m.skips), m.extra_feat_type, m.extra_feat_dim, state=sd)
            for k in t.p:
                t.p[k] = t.p[k].clone().requires_grad_(True)
            self.twins[id(m)] = t
        return self.twins[id(m)]

    def grads(self, m):
        return {k: v.grad for k, v in self.twin(m).p.items()}

    def emb(self, e):
        o = self.R.Embedding(e.in_channels, e.N_freqs)
        o.freq_bands = torch.as_tensor(e.freq_bands).detach().clone().cpu().float()
        o.weights = [float(w) for w in e.weights]
        return o

    @staticmethod
    def _c(t):
        return t if (t is None or not torch.is_tensor(t) or not t.is_cuda) else t.detach().cpu()

    def embed(self, e, x):
        return self.emb(e)(x if not x.is_cuda else self._c(x))

    def pad_to(self, t, width):
        out = torch.zeros((t.shape[0], width))
        out[:, :t.shape[1]] = t
        return out

    def nerf_forward(self, m, inputs, sigma_only=False):
        return self.twin(m)(inputs, sigma_only=sigma_only)

    def nof_forward(self, m, inputs, xyz):
        return self.twin(m)(inputs, xyz)

    def nof_points(self, xyz, ind, embs, m):
        return self.R.nof_inference(xyz, self._c(ind), [self.emb(embs[0]), self.emb(embs[1])], self.twin(m))

    def composite(self, rgbsig, z_vals, rays_d, noise, activation, background):
        N, S = z_vals.shape
        rs = rgbsig.view(N, S, 4)
        nz = torch.zeros(N, S) if noise is None else self._c(noise)
        rgb, depth, weights, alphas = self.R.composite(rs[..., 3], rs[..., :3], self._c(z_vals), self._c(rays_d), nz, activation,
                                                       self._c(background))
        return dict(rgb=rgb, depth=depth, opacity=weights.sum(1), weights=weights, alphas=alphas)


def pad_to(t, width):
    """(P, w) -> (P, width) zero padded on the right (the narrow operands the backward nodes also accept)."""
    if t.shape[1] == width:
        return t
    out = t.new_zeros((t.shape[0], width))
    out[:, :t.shape[1]] = t
    return out


def _check_grads_vs_float64(nets, want32, want64, skip=lambda k: False, label="", fp32_bar=None):
    """fp32_bar: fixed max-rel bar against the fp32 oracle (NeRF-only passes: HIP and the fp32 oracle evaluate the same ReLU
    masks and agree to ~1e-6 where both sit 1e-3 from the float64 truth -- there the fixed 1e-4 is the tighter test).
    The yardstick of a tensor is the larger of its own noise and the MEDIAN noise of its network's tensors: one fp32-vs-float64
    pair is a single draw of a random distance, and on some tensor it comes out several times under the typical one
    (r_moco_global_default, xyz_encoding_8.weight: 1.6e-5 where the network's median is 3e-4 and HIP sits at 2.1e-4)."""
    checked, worst, floor = 0, (0.0, ""), (0.0, "")
    for i, m in enumerate(nets):
        live = [k for k, _ in m.named_parameters() if not skip(k) and want64[f"{i}.{k}"] is not None
                and float(want64[f"{i}.{k}"].abs().max()) > 0.0]
        net_l2 = float(np.median([_l2rel(want32[f"{i}.{k}"], want64[f"{i}.{k}"]) for k in live])) if live else 0.0
        net_mr = float(np.median([relerr(want32[f"{i}.{k}"], want64[f"{i}.{k}"]) for k in live])) if live else 0.0
        for k, p in m.named_parameters():
            key = f"{i}.{k}"
            if skip(k):
                assert p.grad is None, key
                continue
            w64, w32 = want64[key], want32[key]
            if w64 is None or float(w64.abs().max()) == 0.0:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, key
                continue
            assert p.grad is not None, key
            noise_l2, noise_mr = max(_l2rel(w32, w64), net_l2), max(relerr(w32, w64), net_mr)
            e_l2, e_mr32 = _l2rel(p.grad, w64), relerr(p.grad, w32)
            worst, floor = max(worst, (e_l2, key)), max(floor, (noise_l2, key))
            # (NeRF-only passes, fp32_bar given: the multiplier is capped -- ADVICE r4 -- 3 x a 7.6e-3 first-layer floor would let
            #  a 2e-2 error through; the MoCo cases' floors reach 100 % on some tensors and cannot be capped)
            # (HIP shares the fp32 oracle's ReLU masks there and so sits AT the fp32 oracle's own distance from the truth: the cap
            #  cannot go under 1.5 x that distance; the fixed fp32_bar below is what catches a mis-scaled gradient)
            assert e_l2 <= max(TOL, 3 * noise_l2 if fp32_bar is None else min(3 * noise_l2, max(1.5 * noise_l2, 5e-3))), (key, e_l2, noise_l2)
            # max-rel guard against a wrong element.  Its floor is 2e-3, not 1e-4: ONE ReLU unit whose pre-activation rounds to the
            # other side of zero between two fp32 evaluation orders moves a weight-gradient row of the layers in front of it by
            # that sample's whole contribution -- a discrete event (measured 1.4e-4 .. 3.8e-4 of max|dW| at 6144 samples, layers
            # 1-3 only, the layers behind the unit agreeing to 2e-7, with the fp32 backward kernels too: a one-off script, since removed) that
            # the fp32-vs-float64 pair of the same batch need not contain
            assert e_mr32 <= (fp32_bar if fp32_bar is not None else max(2e-3, 3 * noise_mr)), (key, e_mr32, noise_mr)
            checked += 1
    print(f"{label}: end-to-end gradients vs the float64 oracle, worst l2-rel {worst[0]:.2e} at {worst[1]} (the fp32 oracle's own worst "
          f"{floor[0]:.2e} at {floor[1]}; {checked} tensors, each within max(1e-4, 3 x its noise floor))")
    return checked
