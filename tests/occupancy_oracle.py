"""numpy restatement of csrc/mf_occupancy.hip, operation for operation (include/mocoflow_hip.h: mf_occ_build, mf_ray_clip).

The march is fp32 throughout: every numpy operation below works on float32 arrays and so rounds once, exactly where the
kernel rounds (no fused multiply-add); it is vectorised over the rays still marching, the build over the lattice.  The one operation numpy
cannot restate bit for bit is the softplus (log1pf(expf(s)) of the device library): ``activate`` evaluates it in float64, and
``ambiguous`` tells which lattice points lie so close to the threshold that a last-place difference of the device's value
could decide the comparison -- a test draws its values so that none does (relu, and softplus above 20, are exact)."""
import numpy as np

f32 = np.float32
MAX_STEPS = 65536


def activate(sigma, act):
    """float64 activated density of fp32 raw sigma; NaN stays NaN."""
    s = np.asarray(sigma, dtype=np.float32).astype(np.float64)
    if act == "relu":
        return np.where(s < 0, 0.0, s)
    assert act == "softplus", act
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(s > 20, s, np.log1p(np.exp(np.minimum(s, 30.0))))


def ambiguous(sigma, act, tau, ulps=16):
    """Lattice points whose fp32 activated value may fall on either side of tau depending on the last places of the device's
    expf / log1pf (each within a few ulp): |act - tau| <= ulps * ulp(tau).  Never true for relu or for sigma > 20."""
    if act == "relu":
        return np.zeros(np.shape(sigma), dtype=bool)
    s = np.asarray(sigma, dtype=np.float32)
    a = activate(s, act)
    with np.errstate(invalid="ignore"):
        near = np.abs(a - float(tau)) <= ulps * float(np.spacing(np.float32(max(abs(float(tau)), 1e-30))))
    return near & ~(s > 20) & np.isfinite(a)


def active(sigma, act, tau):
    """act(sigma) > tau in fp32, strictly; NaN counts as active."""
    a32 = activate(sigma, act).astype(np.float32)          # relu and sigma > 20: exact; else the float64 softplus, rounded
    with np.errstate(invalid="ignore"):
        return ~(a32 <= np.float32(tau))


def build_dense(sigma, act, tau, dilate):
    """bool (nx-1, ny-1, nz-1): cell (i, j, k) is set iff an active lattice point lies in [i-r, i+1+r] x [j-r, j+1+r] x
    [k-r, k+1+r], clipped to the lattice."""
    on = active(sigma, act, tau)
    r = int(dilate)
    for axis in range(3):
        n = on.shape[axis]
        out = np.zeros(on.shape[:axis] + (n - 1,) + on.shape[axis + 1:], dtype=bool)
        for c in range(n - 1):
            lo, hi = max(c - r, 0), min(c + 1 + r, n - 1)
            out[(slice(None),) * axis + (c,)] = np.take(on, range(lo, hi + 1), axis=axis).any(axis=axis)
        on = out
    return on


def pack(dense):
    """bool (gx, gy, gz) -> uint32 (gx, gy, ceil(gz / 32)): cell k is bit k % 32 of word k / 32, padding bits zero."""
    gx, gy, gz = dense.shape
    wz = (gz + 31) // 32
    padded = np.zeros((gx, gy, wz * 32), dtype=np.uint64)
    padded[:, :, :gz] = dense
    w = (padded.reshape(gx, gy, wz, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32)


def unpack(bits, gz):
    gx, gy, wz = bits.shape
    b = (bits[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return b.reshape(gx, gy, wz * 32)[:, :, :gz].astype(bool)


def build(sigma, act, tau, dilate):
    """(words uint32 (gx, gy, wz), count) of mf_occ_build."""
    dense = build_dense(sigma, act, tau, dilate)
    return pack(dense), int(dense.sum())


def grid_constants(dims, lo, hi, step):
    """(lo, hi, inv_cell, dt) as fp32, the way OccupancyGrid computes them: the cell edge in float64 from the fp32 box,
    inv_cell = fp32(1 / edge), dt = fp32(step * min edge)."""
    lo32, hi32 = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    edge = (hi32.astype(np.float64) - lo32.astype(np.float64)) / np.asarray(dims, dtype=np.float64)
    return lo32, hi32, (1.0 / edge).astype(np.float32), np.float32(float(step) * float(edge.min()))


def max_steps(lo, hi, dt):
    lo, hi = np.asarray(lo, dtype=np.float32).astype(np.float64), np.asarray(hi, dtype=np.float32).astype(np.float64)
    return float(np.floor(np.sqrt(((hi - lo) ** 2).sum()) / float(np.float32(dt))) + 2.0)


def clip(rays, dense, lo, hi, inv_cell, dt):
    """mf_ray_clip: rays (R, >= 8) -> (t_first, t_last) float32, hit uint8."""
    rays = np.asarray(rays, dtype=np.float32)
    dense = np.asarray(dense, dtype=bool)
    G = dense.shape
    lo, hi, inv = (np.asarray(v, dtype=np.float32) for v in (lo, hi, inv_cell))
    dt = np.float32(dt)
    n_max = max_steps(lo, hi, dt)
    assert n_max <= MAX_STEPS and dt > 0 and (lo < hi).all()
    n_max = int(n_max)
    R = rays.shape[0]
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6].copy(), rays[:, 7].copy()
    t_first, t_last, hit = near.copy(), far.copy(), np.zeros(R, dtype=np.uint8)
    fin = np.isfinite(rays[:, :8]).all(1)
    hit[~fin] = 1
    with np.errstate(all="ignore"):
        tmin, tmax = near.copy(), far.copy()
        miss = np.zeros(R, dtype=bool)
        for a in range(3):
            nz = d[:, a] != 0
            da = np.where(nz, d[:, a], f32(1))
            t1, t2 = (lo[a] - o[:, a]) / da, (hi[a] - o[:, a]) / da
            tmin = np.where(nz, np.maximum(tmin, np.minimum(t1, t2)), tmin)
            tmax = np.where(nz, np.minimum(tmax, np.maximum(t1, t2)), tmax)
            miss |= ~nz & ((o[:, a] < lo[a]) | (o[:, a] > hi[a]))
        live = fin & ~miss & ~(tmin > tmax)
        kf, kl = np.full(R, -1, dtype=np.int64), np.full(R, -1, dtype=np.int64)
        cut = np.zeros(R, dtype=bool)
        idx = np.nonzero(live)[0]                       # the rays still marching; the arrays below hold their rows only
        k = 0
        while idx.size:
            t = tmin[idx] + f32(k) * dt
            on_way = t <= tmax[idx]
            idx, t = idx[on_way], t[on_way]
            if k >= n_max:
                cut[idx] = True
                break
            c = []
            for a in range(3):
                fl = np.floor((o[idx, a] + d[idx, a] * t - lo[a]) * inv[a])
                fl = np.where(fl >= 0, fl, f32(0))
                fl = np.where(fl <= f32(G[a] - 1), fl, f32(G[a] - 1))
                c.append(np.minimum(fl.astype(np.int64), G[a] - 1))
            on = idx[dense[c[0], c[1], c[2]]]
            kf[on] = np.where(kf[on] < 0, k, kf[on])
            kl[on] = k
            k += 1
        found = kf >= 0
        hit[found | cut] = 1
        tf = np.maximum(near, (tmin + kf.astype(np.float32) * dt) - dt)
        tl = np.minimum(far, (tmin + kl.astype(np.float32) * dt) + dt)
        t_first = np.where(found, tf, t_first)
        t_last = np.where(found & ~cut, tl, t_last)
    return t_first.astype(np.float32), t_last.astype(np.float32), hit


def lattice(N_grid, aabb):
    """OccupancyGrid.from_field's query points: np.linspace(lo_a, hi_a, N_a) in float64 cast to fp32, x slowest, z fastest."""
    n = (int(N_grid),) * 3 if np.isscalar(N_grid) else tuple(int(v) for v in N_grid)
    aabb = np.asarray(aabb, dtype=np.float64)
    ax = [np.linspace(aabb[0, a], aabb[1, a], n[a]).astype(np.float32) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3), n


def ball_lattice(n, lo, hi, center, radius, inside=5.0, outside=-5.0):
    """A raw-sigma lattice (nx, ny, nz) with ``inside`` at the points within ``radius`` of ``center``."""
    aabb = np.stack([np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)])
    pts, n = lattice(n, aabb)
    dist = np.sqrt(((pts.astype(np.float64) - np.asarray(center, dtype=np.float64)) ** 2).sum(-1))
    return np.where(dist <= radius, inside, outside).astype(np.float32).reshape(n)
