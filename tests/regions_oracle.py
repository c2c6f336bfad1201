"""The contract of matte clean-up (moco_flow_amd/frames.py: clean_mask, mask_regions; csrc/mf_regions.hip) restated in numpy.

    members   alpha >= thres (below: alpha < thres)
    regions   the 8- or 4-connected components of the members of one frame; rows do not wrap
    label     the smallest row-major index y W + x of the region, int32; -1 off the members
    largest   most pixels; ties to the smaller label; no members: all zero
    holes     the 4-connected components of the zeros of a mask without a pixel on the first or last row or column

components() hooks every member to the minimum over its neighbourhood and jumps pointers until nothing changes;
components_tiled() follows the kernels' decomposition instead -- components per tile, then the seam rule (W, NW, N, NE into
another tile) through a sequential union-find -- and must give the same labels: that holds the decomposition without a GPU."""
import numpy as np

OFFSETS = {4: ((-1, 0), (0, -1), (0, 1), (1, 0)),
           8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def members(alpha, thres=196, below=False):
    a = np.asarray(alpha).astype(np.int64)
    return a < thres if below else a >= thres


def components(fg, conn=8):
    """fg: (H, W) bool -> (H, W) int32 labels: the smallest row-major index of the pixel's region, -1 off the members."""
    fg = np.asarray(fg, dtype=bool)
    H, W = fg.shape
    n = H * W
    if n == 0:
        return np.full((H, W), -1, dtype=np.int32)
    lab = np.where(fg, np.arange(n, dtype=np.int64).reshape(H, W), n)
    pad = np.full((H + 2, W + 2), n, dtype=np.int64)
    while True:
        pad[1:-1, 1:-1] = lab
        m = lab.copy()
        for dy, dx in OFFSETS[conn]:
            np.minimum(m, pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W], out=m)
        flat = np.append(np.where(fg, m, n).ravel(), n)          # entry n: "no region", its own parent
        while True:                                               # every value is a pixel of the same region: jump
            nxt = flat[flat]
            if np.array_equal(nxt, flat):
                break
            flat = nxt
        new = flat[:n].reshape(H, W)
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(fg, lab, -1).astype(np.int32)


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def _unite(parent, a, b):
    ra, rb = _find(parent, a), _find(parent, b)
    if ra != rb:
        parent[max(ra, rb)] = min(ra, rb)


def _seam_unions_thinned(fg, conn, th, tw):
    """The unions reg_seam_kernel makes: below a horizontal seam N only at the first column that the run below and the run above
    share, a diagonal only where neither pixel beside it is a member; across a vertical seam W always, a diagonal only where
    exactly one of the two pixels of the row is a member and the pixel above it is not."""
    H, W = fg.shape
    at = lambda y, x: 0 <= y < H and 0 <= x < W and bool(fg[y, x])
    for y in range(th, H, th):
        for x in range(W):
            if not fg[y, x]:
                continue
            aN, aW, aE, bW, bE = at(y - 1, x), at(y - 1, x - 1), at(y - 1, x + 1), at(y, x - 1), at(y, x + 1)
            if aN and not (bW and aW):
                yield (y, x), (y - 1, x)
            if conn == 8 and not aN:
                if aW and not bW:
                    yield (y, x), (y - 1, x - 1)
                if aE and not bE:
                    yield (y, x), (y - 1, x + 1)
    for x in range(tw, W, tw):
        for y in range(H):
            m, mW = at(y, x), at(y, x - 1)
            if m and mW:
                yield (y, x), (y, x - 1)
            if conn == 8 and y > 0 and m != mW:
                aN, aW = at(y - 1, x), at(y - 1, x - 1)
                if m and aW and not aN:
                    yield (y, x), (y - 1, x - 1)
                if mW and aN and not aW:
                    yield (y, x - 1), (y - 1, x)


def components_tiled(fg, conn, th, tw, thinned=False):
    """The kernels' decomposition: the components of every th x tw tile, written as global indices; then a member whose W, NW,
    N or NE neighbour (4-connectivity: W, N) is a member of another tile unites with it.  thinned: only the unions that
    reg_seam_kernel makes of those (one per pair of touching runs)."""
    fg = np.asarray(fg, dtype=bool)
    H, W = fg.shape
    parent = np.arange(H * W, dtype=np.int64)
    for y0 in range(0, H, th):
        for x0 in range(0, W, tw):
            tile = fg[y0:y0 + th, x0:x0 + tw]
            h, w = tile.shape
            loc = components(tile, conn)
            glob = (y0 + loc // w) * W + x0 + loc % w
            ys, xs = np.nonzero(tile)
            parent[(y0 + ys) * W + x0 + xs] = glob[ys, xs]
    steps = ((0, -1), (-1, 0)) if conn == 4 else ((0, -1), (-1, -1), (-1, 0), (-1, 1))
    if thinned:
        for (y, x), (yy, xx) in _seam_unions_thinned(fg, conn, th, tw):
            _unite(parent, y * W + x, yy * W + xx)
    else:
        for y, x in zip(*np.nonzero(fg)):
            for dy, dx in steps:
                yy, xx = y + dy, x + dx
                if 0 <= yy and 0 <= xx < W and fg[yy, xx] and (yy // th, xx // tw) != (y // th, x // tw):
                    _unite(parent, y * W + x, yy * W + xx)
    out = np.full(H * W, -1, dtype=np.int32)
    for g in np.flatnonzero(fg.ravel()):
        out[g] = _find(parent, g)
    return out.reshape(H, W)


def table(labels):
    """labels: (F, H, W) -> (counts (F,) int64, rows (sum counts, 7) int32: frame, label, area, x0, y0, x1, y1 inclusive, in
    (frame, label) order)."""
    labels = np.asarray(labels)
    F, H, W = labels.shape
    rows, counts = [], np.zeros(F, dtype=np.int64)
    for f in range(F):
        lab = labels[f].ravel()
        idx = np.flatnonzero(lab >= 0)
        ids, inv, area = np.unique(lab[idx], return_inverse=True, return_counts=True)
        counts[f] = len(ids)
        if len(ids) == 0:
            continue
        ys, xs = idx // W, idx % W
        x0 = np.full(len(ids), W); y0 = np.full(len(ids), H); x1 = np.full(len(ids), -1); y1 = np.full(len(ids), -1)
        np.minimum.at(x0, inv, xs); np.minimum.at(y0, inv, ys); np.maximum.at(x1, inv, xs); np.maximum.at(y1, inv, ys)
        rows.append(np.stack([np.full(len(ids), f), ids, area, x0, y0, x1, y1], axis=1))
    rows = np.concatenate(rows, axis=0) if rows else np.zeros((0, 7))
    return counts, rows.astype(np.int32)


def regions(alpha, thres=196, conn=8, below=False):
    """alpha: (F, H, W) bytes -> (labels (F, H, W) int32, counts, table)."""
    alpha = np.asarray(alpha)
    labels = np.stack([components(members(a, thres, below), conn) for a in alpha]) if len(alpha) else np.zeros(alpha.shape, np.int32)
    return (labels,) + table(labels)


def fill_holes(mask):
    """mask: (H, W), non-zero = inside -> uint8 {0, 255}: the mask plus its holes."""
    M = np.asarray(mask) != 0
    H, W = M.shape
    out = M.copy()
    if H > 2 and W > 2:
        lab = components(~M, 4)
        border = np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]])
        out |= (lab >= 0) & ~np.isin(lab, border[border >= 0])
    return out.astype(np.uint8) * 255


def select(labels, largest=True, min_area=0):
    """labels: (H, W) of one frame -> uint8 {0, 255}."""
    lab = np.asarray(labels)
    ids, area = np.unique(lab[lab >= 0], return_counts=True)
    if len(ids) == 0:
        return np.zeros(lab.shape, dtype=np.uint8)
    keep = ids[area >= min_area]
    if largest:
        win = ids[np.argmax(area)]                               # the first maximum: ids ascend, ties go to the smaller label
        keep = keep[keep == win]
    return np.isin(lab, keep).astype(np.uint8) * 255


def clean_mask(alpha, thres=196, largest=True, min_area=0, fill=False, conn=8):
    """alpha: (F, H, W) bytes -> (F, H, W) uint8 {0, 255}."""
    out = []
    for a in np.asarray(alpha):
        m = select(components(members(a, thres), conn), largest, min_area)
        out.append(fill_holes(m) if fill else m)
    return np.stack(out) if out else np.zeros(np.asarray(alpha).shape, dtype=np.uint8)


# ---------------------------------------------------------------- patterns the tests share (bool (H, W))
def seam_pairs(th, tw):
    """(name, pixel a, pixel b, joined under 4-connectivity): two pixels that touch only across a tile seam (all join under 8)."""
    return (("N across a horizontal seam", (th - 1, 5), (th, 5), True),
            ("W across a vertical seam", (3, tw - 1), (3, tw), True),
            ("NW across a four-tile corner", (th - 1, tw - 1), (th, tw), False),
            ("NE across a four-tile corner", (th - 1, tw), (th, tw - 1), False),
            ("NE from a tile's last column, away from a corner", (5, tw), (6, tw - 1), False),
            ("N across the second horizontal seam", (2 * th - 1, tw + 1), (2 * th, tw + 1), True),
            ("NE from the last column across the second horizontal seam", (2 * th - 1, tw), (2 * th, tw - 1), False))


def serpentine(H, W):
    """Every even row, joined alternately at the right and the left end: one region through every tile, label 0, of
    serpentine_area(H, W) pixels under either connectivity."""
    m = np.zeros((H, W), dtype=bool)
    m[0::2] = True
    m[1::4, W - 1] = True
    m[3::4, 0] = True
    return m


def serpentine_area(H, W):
    return (H + 1) // 2 * W + H // 2


def comb(H, W):
    """Teeth in every even column that meet only in the last row: one region, label 0."""
    m = np.zeros((H, W), dtype=bool)
    m[:, 0::2] = True
    m[H - 1] = True
    return m


def nested_us(H, W):
    """U k: columns 2 k and W - 1 - 2 k from the first row down to row H - 1 - 2 k, joined along that row: the two arms of a U
    meet at its bottom only; U k is one region of label 2 k."""
    m = np.zeros((H, W), dtype=bool)
    k = 0
    while 2 * k + 2 <= W - 1 - 2 * k and H - 1 - 2 * k >= 1:
        xl, xr, yb = 2 * k, W - 1 - 2 * k, H - 1 - 2 * k
        m[:yb + 1, xl] = True
        m[:yb + 1, xr] = True
        m[yb, xl:xr + 1] = True
        k += 1
    return m


def spirals(H, W):
    """Two interleaved spirals: a one-pixel wall winding inwards with a corridor of three, and the corridor's centre line."""
    a = np.zeros((H, W), dtype=bool)
    y, x, dy, dx = 0, 0, 0, 1
    a[0, 0] = True
    turns = 0
    while turns < 2:
        ny, nx = y + dy, x + dx
        fy, fx = y + 4 * dy, x + 4 * dx
        if not (0 <= ny < H and 0 <= nx < W) or (0 <= fy < H and 0 <= fx < W and a[fy, fx]) or a[ny, nx]:
            dy, dx = dx, -dy
            turns += 1
            continue
        y, x, turns = ny, nx, 0
        a[y, x] = True
    pad = np.pad(a, 1, constant_values=True)
    near = np.zeros((H, W), dtype=bool)
    for oy in range(3):
        for ox in range(3):
            near |= pad[oy:oy + H, ox:ox + W]
    return a | ~near
