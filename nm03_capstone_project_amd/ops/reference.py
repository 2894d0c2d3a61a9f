"""Plain-PyTorch fp32 references of each pipeline op (the numerics oracle for the HIP kernels,
independent of the C++ golden model). All functions take/return torch tensors on any device."""
import math

import torch
import torch.nn.functional as F


def norm_clip(x, low=0.5, high=2.5, vmin=0.0, vmax=10000.0, cmin=0.68, cmax=4000.0):
    t = (x.float() - vmin) / (vmax - vmin)
    t = t * (high - low) + low
    return t.clamp(cmin, cmax)


def median(img, k=7):
    """Exact k×k median with replicate (clamp-to-edge) padding; img [H, W] float."""
    r = k // 2
    x = F.pad(img[None, None].float(), (r, r, r, r), mode="replicate")
    patches = F.unfold(x, k)  # [1, k*k, H*W]
    return patches.median(dim=1).values.reshape(img.shape)


def gaussian_kernel2d(sigma=0.5, mask=9, dtype=torch.float64):
    r = mask // 2
    ax = torch.arange(-r, r + 1, dtype=dtype)
    g = torch.exp(-(ax[:, None] ** 2 + ax[None, :] ** 2) / (2 * sigma * sigma))
    return g / g.sum()


def sharpen(img, gain=2.0, sigma=0.5, mask=9):
    """Unsharp mask s = c + gain (c − G∗c) in float64 with replicate padding (FAST's 2D form)."""
    r = mask // 2
    x = img.double()[None, None]
    k = gaussian_kernel2d(sigma, mask).to(x.device)[None, None]
    b = F.conv2d(F.pad(x, (r, r, r, r), mode="replicate"), k)[0, 0]
    c = img.double()
    return c + gain * (c - b)


def band(s, lo=0.74, hi=0.91):
    return (s >= lo) & (s <= hi)


def threshold(x, lo, hi):
    """BinaryThresholding reference: lo ≤ x ≤ hi → 1 (uint8)."""
    return ((x >= lo) & (x <= hi)).to(torch.uint8)


def dilate(mask, size=3):
    r = size // 2
    x = mask.float()[None, None]
    return (F.max_pool2d(x, size, stride=1, padding=r)[0, 0] > 0.5)


def erode(mask, size=3):
    # max_pool2d pads with -inf, i.e. out-of-image samples never win: "ignored" (App. A.7).
    r = size // 2
    x = (1.0 - mask.float())[None, None]
    return ~(F.max_pool2d(x, size, stride=1, padding=r)[0, 0] > 0.5)


def disc_se(size, dims=2):
    """The digital disc (dims=2) / ball (dims=3) of radius size // 2: offsets with |d|² ≤ r²."""
    r = size // 2
    ax = torch.arange(-r, r + 1, dtype=torch.int64)
    grids = torch.meshgrid(*([ax] * dims), indexing="ij")
    return sum(g * g for g in grids) <= r * r


def dilate_disc(mask, size=3):
    """Binary dilation with the disc SE as a conv2d count (zero padding = out-of-image ignored)."""
    r = size // 2
    k = disc_se(size).to(torch.float64)[None, None].to(mask.device)
    return F.conv2d(mask.to(torch.float64)[None, None], k, padding=r)[0, 0] > 0.5


def erode_disc(mask, size=3):
    """Binary erosion with the disc SE: every in-image sample under the disc set. Out-of-image samples
    are ignored: the count of set samples equals the count of in-image samples under the disc."""
    r = size // 2
    k = disc_se(size).to(torch.float64)[None, None].to(mask.device)
    hits = F.conv2d(mask.to(torch.float64)[None, None], k, padding=r)[0, 0]
    inside = F.conv2d(torch.ones_like(mask, dtype=torch.float64)[None, None], k, padding=r)[0, 0]
    return hits > inside - 0.5


def dilate_ball(mask, size=7):
    """3D binary dilation with the ball SE as a conv3d count, [D, H, W]."""
    r = size // 2
    k = disc_se(size, 3).to(torch.float64)[None, None].to(mask.device)
    return F.conv3d(mask.to(torch.float64)[None, None], k, padding=r)[0, 0] > 0.5


def border(mask, radius=2):
    return mask & ~erode(mask, 2 * radius + 1)


def region_grow(bnd, seeds, connectivity=4):
    """Geodesic reconstruction: iterate R ← band ∧ dilate(R) from the in-band seeds to a fixpoint."""
    h, w = bnd.shape
    reg = torch.zeros_like(bnd)
    for (x, y, *_rest) in seeds:
        if 0 <= x < w and 0 <= y < h and bnd[y, x]:
            reg[y, x] = True
    if connectivity == 4:
        k = torch.tensor([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=torch.float32, device=bnd.device)
    else:
        k = torch.ones((3, 3), dtype=torch.float32, device=bnd.device)
    while True:
        grown = F.conv2d(reg.float()[None, None], k[None, None], padding=1)[0, 0] > 0
        nxt = grown & bnd
        if torch.equal(nxt, reg):
            return reg
        reg = nxt


def render_gray(values, lo, hi, out_w=512, out_h=512, nearest=False):
    """Bilinear 2× (generally: fit) render of an [H, W] float image onto out_h×out_w, f32 math
    in the contract order (pixel_math.h), window [lo, hi] → uint8. `nearest`: the source pixel under
    each canvas pixel's centre instead (--render-filter nearest)."""
    h, w = values.shape
    scale = min(out_w / w, out_h / h)
    ox, oy = (out_w - w * scale) / 2, (out_h - h * scale) / 2
    dev = values.device
    u = torch.arange(out_w, device=dev, dtype=torch.float32)
    v = torch.arange(out_h, device=dev, dtype=torch.float32)
    sx = (u + 0.5 - ox) * (1.0 / scale)
    sy = (v + 0.5 - oy) * (1.0 / scale)
    fx, fy = sx - 0.5, sy - 0.5
    x0, y0 = torch.floor(fx), torch.floor(fy)
    wx, wy = fx - x0, fy - y0
    x0i, y0i = x0.long(), y0.long()
    xa, xb = x0i.clamp(0, w - 1), (x0i + 1).clamp(0, w - 1)
    ya, yb = y0i.clamp(0, h - 1), (y0i + 1).clamp(0, h - 1)
    a = values[ya][:, xa]
    b = values[ya][:, xb]
    c = values[yb][:, xa]
    d = values[yb][:, xb]
    top = (1 - wx) * a + wx * b
    bot = (1 - wx) * c + wx * d
    val = (1 - wy)[:, None] * top + wy[:, None] * bot
    if nearest:
        val = values[torch.floor(sy).long().clamp(0, h - 1)][:, torch.floor(sx).long().clamp(0, w - 1)]
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(hi - lo, dtype=torch.float32) if hi > lo else torch.tensor(0.0)
    g = ((val - lo) * inv.to(val.device)).clamp(0, 1)
    out = torch.floor(g * 255 + 0.5).to(torch.uint8)
    inside = ((sx >= 0) & (sx < w))[None, :] & ((sy >= 0) & (sy < h))[:, None]
    return torch.where(inside, out, torch.zeros_like(out))


def render_labels(label, brd, fill=153, border_value=255, out_w=512, out_h=512):
    h, w = label.shape
    scale = min(out_w / w, out_h / h)
    ox, oy = (out_w - w * scale) / 2, (out_h - h * scale) / 2
    dev = label.device
    sx = (torch.arange(out_w, device=dev, dtype=torch.float32) + 0.5 - ox) / scale
    sy = (torch.arange(out_h, device=dev, dtype=torch.float32) + 0.5 - oy) / scale
    xi = torch.floor(sx).long().clamp(0, w - 1)
    yi = torch.floor(sy).long().clamp(0, h - 1)
    lab = label[yi][:, xi]
    bd = brd[yi][:, xi]
    out = torch.where(bd, torch.full_like(lab, border_value, dtype=torch.uint8),
                      torch.where(lab, torch.full_like(lab, fill, dtype=torch.uint8),
                                  torch.zeros_like(lab, dtype=torch.uint8)))
    inside = ((sx >= 0) & (sx < w))[None, :] & ((sy >= 0) & (sy < h))[:, None]
    return torch.where(inside, out, torch.zeros_like(out))


def overlay(values, lo, hi, label, brd, spacing=(1.0, 1.0), out_w=512, out_h=512, nearest=False, fill_a=153,
            border_a=255, color=(0, 255, 0)):
    """Overlay canvas [out_h, out_w, 3] uint8: the gray render of `values` [H, W] (window [lo, hi])
    with `color` blended over it per channel as (a·C + (255 − a)·g + 127) // 255 in integers, where
    a = border_a under a set `brd` pixel, else fill_a under a set `label` pixel, else 0 (both bool
    [H, W], sampled nearest). The slice is fitted to the canvas preserving its physical aspect
    (`spacing` = (x, y) mm per pixel) and centred; pixels outside it stay black."""
    h, w = values.shape
    dev = values.device
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    spx, spy = (float(torch.tensor(s, dtype=torch.float32)) for s in spacing)
    ew, eh = w * spx, h * spy
    scale = min(out_w / ew, out_h / eh)
    dw, dh = ew * scale, eh * scale
    ox, oy = f32((out_w - dw) * 0.5), f32((out_h - dh) * 0.5)
    invx, invy = f32(w / dw), f32(h / dh)
    sx = ((torch.arange(out_w, device=dev, dtype=torch.float32) + 0.5) - ox) * invx
    sy = ((torch.arange(out_h, device=dev, dtype=torch.float32) + 0.5) - oy) * invy
    inside = ((sx >= 0) & (sx < w))[None, :] & ((sy >= 0) & (sy < h))[:, None]
    xn, yn = torch.floor(sx).long().clamp(0, w - 1), torch.floor(sy).long().clamp(0, h - 1)
    v = values.float()
    if nearest:
        val = v[yn][:, xn]
    else:
        fx, fy = sx - 0.5, sy - 0.5
        x0, y0 = torch.floor(fx), torch.floor(fy)
        wx, wy = (fx - x0)[None, :], (fy - y0)[:, None]
        xa, xb = x0.long().clamp(0, w - 1), (x0.long() + 1).clamp(0, w - 1)
        ya, yb = y0.long().clamp(0, h - 1), (y0.long() + 1).clamp(0, h - 1)
        top = (1 - wx) * v[ya][:, xa] + wx * v[ya][:, xb]
        bot = (1 - wx) * v[yb][:, xa] + wx * v[yb][:, xb]
        val = (1 - wy) * top + wy * bot
    inv = f32(1.0) / f32(hi - lo) if hi > lo else f32(0.0)
    g = torch.floor(((val - lo) * inv).clamp(0, 1) * 255 + 0.5).to(torch.int32)
    a = torch.where(brd.bool()[yn][:, xn], border_a, torch.where(label.bool()[yn][:, xn], fill_a, 0)).to(torch.int32)
    g = torch.where(inside, g, torch.zeros_like(g))
    a = torch.where(inside, a, torch.zeros_like(a))
    c = torch.tensor([int(k) for k in color], dtype=torch.int32, device=dev)
    out = (a[..., None] * c + (255 - a[..., None]) * g[..., None] + 127) // 255
    return out.to(torch.uint8)


def measure(dilated, region, raw, connectivity=8, pixel_type="u16", stored_bits=16):
    """The measurement record (nm03/measure.h) of one slice in NumPy + scipy.ndimage.label: a third
    implementation beside the golden model's flood fill and the K7 kernel's union-find. `dilated`,
    `region`: [H, W] masks (torch or NumPy, any device); `raw`: [H, W] 16-bit storage. Components are
    labelled at `connectivity` (4 | 8); holes are the components of the COMPLEMENT of the 1-pixel-padded
    mask at the dual connectivity, minus the outer one. Returns the dict of integers ops.measure_mask gives."""
    import numpy as np
    from scipy import ndimage  # imported lazily: only this reference needs SciPy

    def to_np(t):
        return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    m = to_np(dilated).astype(bool)
    h, w = m.shape
    cross = ndimage.generate_binary_structure(2, 1)
    square = ndimage.generate_binary_structure(2, 2)
    lab, ncomp = ndimage.label(m, structure=square if connectivity == 8 else cross)
    sizes = np.bincount(lab.ravel())[1:] if ncomp else np.zeros(0, dtype=np.int64)
    _, nbg = ndimage.label(~np.pad(m, 1), structure=cross if connectivity == 8 else square)
    ys, xs = np.nonzero(m)
    p = np.pad(m, 1)
    core = p[1:-1, 1:-1]
    edges = sum(int((core & ~nb).sum()) for nb in (p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]))
    v = to_np(raw).view(np.uint16).astype(np.int64)
    sh = 16 - int(stored_bits)
    if pixel_type == "i16":
        v = ((v << sh) & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64) >> sh
    else:
        v = v & (0xFFFF >> sh)
    under = v[m]
    any_px = bool(m.any())
    return {
        "area_px": int(m.sum()),
        "region_px": int(to_np(region).astype(bool).sum()),
        "bbox": [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())] if any_px else [-1, -1, -1, -1],
        "sum_x": int(xs.sum()),
        "sum_y": int(ys.sum()),
        "perimeter_edges": edges,
        "components": int(ncomp),
        "largest_px": int(sizes.max()) if ncomp else 0,
        "holes": int(nbg) - 1,
        "raw_sum": int(under.sum()) if any_px else 0,
        "raw_min": int(under.min()) if any_px else 0,
        "raw_max": int(under.max()) if any_px else 0,
    }


def measure_diameters(dilated, connectivity=8):
    """The diameter record (nm03/measure.h SliceDiameters) of one mask [H, W] (torch or NumPy) in NumPy +
    scipy.ndimage.label: a third method beside the golden model (column extremes) and the K9 kernel (row
    extremes). The lesion is the label with the largest count (`argmax` of `bincount` takes the first,
    and labels are numbered in raster order of their first pixel); the candidates are the vertices of
    its convex hull (Andrew's monotone chain in exact integers, collinear points dropped); the pair and
    the projection extremes are brute force over them with the record's tie-breaks."""
    import numpy as np
    from scipy import ndimage

    m = (dilated.detach().cpu().numpy() if isinstance(dilated, torch.Tensor) else np.asarray(dilated)).astype(bool)
    structure = ndimage.generate_binary_structure(2, 2 if connectivity == 8 else 1)
    lab, ncomp = ndimage.label(m, structure=structure)
    rec = {"lesion_px": 0, "lesion_first": [-1, -1], "major_px2": 0, "major": [-1] * 4, "perp_extent": 0, "perp": [-1] * 4}
    if ncomp == 0:
        return rec
    sizes = np.bincount(lab.ravel())[1:]
    k = int(np.argmax(sizes)) + 1
    ys, xs = np.nonzero(lab == k)  # raster order
    rec["lesion_px"] = int(sizes[k - 1])
    rec["lesion_first"] = [int(xs[0]), int(ys[0])]
    pts = sorted(set(zip(xs.tolist(), ys.tolist())))  # (x, y), sorted by x then y

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    if len(pts) > 2:
        lower, upper = [], []
        for p in pts:
            while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
                lower.pop()
            lower.append(p)
        for p in reversed(pts):
            while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
                upper.pop()
            upper.append(p)
        pts = lower[:-1] + upper[:-1]
    hull = sorted((y, x) for x, y in pts)  # (y, x) order
    best = None
    for i, (ya, xa) in enumerate(hull):
        for yb, xb in hull[i:]:
            d2 = (xb - xa) ** 2 + (yb - ya) ** 2
            if best is None or d2 > best[0]:
                best = (d2, xa, ya, xb, yb)
    d2, xa, ya, xb, yb = best
    dx, dy = xb - xa, yb - ya
    proj = [(-dy * x + dx * y, y, x) for y, x in hull]
    pmin, pmax = min(p[0] for p in proj), max(p[0] for p in proj)
    _, yc, xc = min(p for p in proj if p[0] == pmin)
    _, yd, xd = min(p for p in proj if p[0] == pmax)
    rec.update(major_px2=int(d2), major=[xa, ya, xb, yb], perp_extent=int(pmax - pmin), perp=[xc, yc, xd, yd])
    return rec


def measure_volume(dilated, region, raw, connectivity=26, pixel_type="u16", stored_bits=16):
    """The volume record (nm03/measure.h VolumeMeasure) in NumPy + scipy.ndimage.label: a third
    implementation beside the golden model's flood fill and the K8 kernels' union-find. `dilated`,
    `region`: [D, H, W] masks (torch or NumPy, any device); `raw`: [D, H, W] 16-bit storage. Components
    are labelled at `connectivity` (6 | 26: generate_binary_structure(3, 1 | 3)); cavities are the
    components of the COMPLEMENT of the 1-voxel-padded mask at the dual connectivity, minus the outer
    one. The Euler number comes from the window counts over the zero-padded volume: n3 voxels, n2
    face-adjacent pairs, n1 2×2 windows (three orientations), n0 2×2×2 windows, a pair or window
    counting when ANY of its voxels is set at 26-connectivity (euler = n0 − n1 + n2 − n3) and when ALL
    are at 6-connectivity (euler = n3 − n2 + n1 − n0). Returns the dict ops.measure_volume gives."""
    import numpy as np
    from scipy import ndimage  # imported lazily: only this reference needs SciPy

    def to_np(t):
        return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    if connectivity not in (6, 26):
        raise ValueError("connectivity must be 6 or 26")
    m = to_np(dilated).astype(bool)
    if m.ndim != 3:
        raise ValueError("dilated must be [D, H, W]")
    s6, s26 = ndimage.generate_binary_structure(3, 1), ndimage.generate_binary_structure(3, 3)
    lab, ncomp = ndimage.label(m, structure=s26 if connectivity == 26 else s6)
    sizes = np.bincount(lab.ravel())[1:] if ncomp else np.zeros(0, dtype=np.int64)
    _, nbg = ndimage.label(~np.pad(m, 1), structure=s6 if connectivity == 26 else s26)
    zs, ys, xs = np.nonzero(m)
    p = np.pad(m, 1)
    core = p[1:-1, 1:-1, 1:-1]
    faces = [int((core & ~lo).sum()) + int((core & ~hi).sum())
             for lo, hi in ((p[1:-1, 1:-1, :-2], p[1:-1, 1:-1, 2:]), (p[1:-1, :-2, 1:-1], p[1:-1, 2:, 1:-1]),
                            (p[:-2, 1:-1, 1:-1], p[2:, 1:-1, 1:-1]))]
    # Windows of the padded volume, named by their highest corner: q[z, y, x] ↔ voxels z − 1 … z etc.
    hi, lo = slice(1, None), slice(None, -1)
    comb = np.logical_and if connectivity == 6 else np.logical_or

    def count(*parts):
        acc = parts[0]
        for q in parts[1:]:
            acc = comb(acc, q)
        return int(acc.sum())

    v = {(dz, dy, dx): p[(lo if dz else hi), (lo if dy else hi), (lo if dx else hi)]
         for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
    n3 = int(m.sum())
    n2 = count(v[0, 0, 0], v[0, 0, 1]) + count(v[0, 0, 0], v[0, 1, 0]) + count(v[0, 0, 0], v[1, 0, 0])
    n1 = (count(v[0, 0, 0], v[0, 0, 1], v[0, 1, 0], v[0, 1, 1]) + count(v[0, 0, 0], v[0, 0, 1], v[1, 0, 0], v[1, 0, 1]) +
          count(v[0, 0, 0], v[0, 1, 0], v[1, 0, 0], v[1, 1, 0]))
    n0 = count(*v.values())
    euler = n3 - n2 + n1 - n0 if connectivity == 6 else n0 - n1 + n2 - n3
    raw_v = to_np(raw).view(np.uint16).astype(np.int64)
    sh = 16 - int(stored_bits)
    if pixel_type == "i16":
        raw_v = ((raw_v << sh) & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64) >> sh
    else:
        raw_v = raw_v & (0xFFFF >> sh)
    under = raw_v[m]
    any_vox = bool(m.any())
    return {
        "volume_vox": n3,
        "region_vox": int(to_np(region).astype(bool).sum()),
        "bbox": ([int(xs.min()), int(ys.min()), int(zs.min()), int(xs.max()), int(ys.max()), int(zs.max())]
                 if any_vox else [-1] * 6),
        "sum_x": int(xs.sum()),
        "sum_y": int(ys.sum()),
        "sum_z": int(zs.sum()),
        "faces_x": faces[0],
        "faces_y": faces[1],
        "faces_z": faces[2],
        "components": int(ncomp),
        "largest_vox": int(sizes.max()) if ncomp else 0,
        "cavities": int(nbg) - 1,
        "euler": int(euler),
        "raw_sum": int(under.sum()) if any_vox else 0,
        "raw_min": int(under.min()) if any_vox else 0,
        "raw_max": int(under.max()) if any_vox else 0,
    }


def measure_volume_lesions(dilated, region, raw, max_lesions, connectivity=26, pixel_type="u16", stored_bits=16):
    """(record, lesions) as ops.measure_volume_lesions gives them, in NumPy + scipy.ndimage.label: the
    record is measure_volume's; the lesions are the labels' statistics — ndimage.label numbers the
    components in the raster order of their first voxels, so a stable sort by size gives the order
    rule — with the open faces by shifted comparisons against the zero-padded mask."""
    import numpy as np
    from scipy import ndimage

    def to_np(t):
        return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    if not 1 <= int(max_lesions) <= 64:
        raise ValueError("max_lesions must be 1..64")
    rec = measure_volume(dilated, region, raw, connectivity, pixel_type, stored_bits)
    m = to_np(dilated).astype(bool)
    lab, ncomp = ndimage.label(m, structure=ndimage.generate_binary_structure(3, 3 if connectivity == 26 else 1))
    sizes = np.bincount(lab.ravel(), minlength=ncomp + 1)[1:]
    order = np.argsort(-sizes, kind="stable")[:int(max_lesions)]
    raw_v = to_np(raw).view(np.uint16).astype(np.int64)
    sh = 16 - int(stored_bits)
    if pixel_type == "i16":
        raw_v = ((raw_v << sh) & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64) >> sh
    else:
        raw_v = raw_v & (0xFFFF >> sh)
    p = np.pad(m, 1)
    core = (slice(1, -1),) * 3
    # open[axis][side]: mask voxels whose neighbour on that side is not mask (or is the frame)
    opened = []
    for axis in (2, 1, 0):  # x, y, z
        lo = [slice(1, -1)] * 3
        hi = [slice(1, -1)] * 3
        lo[axis], hi[axis] = slice(None, -2), slice(2, None)
        opened.append((p[core] & ~p[tuple(lo)], p[core] & ~p[tuple(hi)]))
    lesions = []
    for i in order:
        sel = lab == i + 1
        zs, ys, xs = np.nonzero(sel)  # raster order
        under = raw_v[sel]
        faces = [int((a & sel).sum()) + int((b & sel).sum()) for a, b in opened]
        lesions.append({
            "voxels": int(sizes[i]),
            "first": [int(xs[0]), int(ys[0]), int(zs[0])],
            "bbox": [int(xs.min()), int(ys.min()), int(zs.min()), int(xs.max()), int(ys.max()), int(zs.max())],
            "sum_x": int(xs.sum()), "sum_y": int(ys.sum()), "sum_z": int(zs.sum()),
            "faces_x": faces[0], "faces_y": faces[1], "faces_z": faces[2],
            "raw_sum": int(under.sum()), "raw_min": int(under.min()), "raw_max": int(under.max()),
        })
    return rec, lesions


def measure_volume_diameters(dilated, max_lesions, spacing_um=(1000, 1000, 1000), connectivity=26):
    """The diameter dicts ops.measure_volume_diameters gives, in NumPy + scipy.ndimage.label: the lesions
    in measure_volume_lesions' order; per lesion the voxels with an open 6-face in raster order, and the
    squared distances of all their pairs in int64, a block of rows at a time. The first row that reaches
    the maximum and the first column in it are the pair the tie rule asks for."""
    import numpy as np
    from scipy import ndimage

    m = (dilated.detach().cpu().numpy() if isinstance(dilated, torch.Tensor) else np.asarray(dilated)).astype(bool)
    if not 1 <= int(max_lesions) <= 64:
        raise ValueError("max_lesions must be 1..64")
    if m.ndim != 3:
        raise ValueError("dilated must be [D, H, W]")
    ux, uy, uz = (int(v) for v in spacing_um)
    if min(ux, uy, uz) < 1:
        raise ValueError("spacing_um must be three integers of at least 1")
    d, h, w = m.shape
    if max((w - 1) * ux, (h - 1) * uy, (d - 1) * uz) >= 2 ** 31:
        raise ValueError("the volume is too long to measure in micrometres")
    lab, ncomp = ndimage.label(m, structure=ndimage.generate_binary_structure(3, 3 if connectivity == 26 else 1))
    sizes = np.bincount(lab.ravel(), minlength=ncomp + 1)[1:]
    order = np.argsort(-sizes, kind="stable")[:int(max_lesions)]
    p = np.pad(m, 1)
    closed = (p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[:-2, 1:-1, 1:-1] &
              p[2:, 1:-1, 1:-1])
    out = []
    for i in order:
        sel = lab == i + 1
        zs, ys, xs = (v.astype(np.int64) for v in np.nonzero(sel & ~closed))  # raster order
        n = len(zs)
        X, Y, Z = xs * ux, ys * uy, zs * uz
        best3 = (-1, 0, 0)
        best2 = (-1, 0, 0)
        step = max(1, (1 << 22) // n)
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            dxy = (X[r0:r1, None] - X[None, :]) ** 2 + (Y[r0:r1, None] - Y[None, :]) ** 2
            d3 = dxy.astype(np.uint64) + ((Z[r0:r1, None] - Z[None, :]) ** 2).astype(np.uint64)  # three squares below 2^62
            dxy = np.where(zs[r0:r1, None] == zs[None, :], dxy, -1)
            for arr, which in ((d3, 3), (dxy, 2)):
                rowmax = arr.max(axis=1)
                top = int(rowmax.max())
                cur = best3 if which == 3 else best2
                if top > cur[0]:
                    a = int(np.argmax(rowmax == top))
                    b = int(np.argmax(arr[a] == top))
                    if which == 3:
                        best3 = (top, r0 + a, b)
                    else:
                        best2 = (top, r0 + a, b)
        ma, mb = sorted(best3[1:])
        aa, ab = sorted(best2[1:])
        dx, dy = int(xs[ab] - xs[aa]), int(ys[ab] - ys[aa])
        plane = zs == zs[aa]
        px, py = xs[plane], ys[plane]
        proj = -dy * px + dx * py
        c, e = int(np.argmin(proj)), int(np.argmax(proj))  # the first in raster order at each end
        out.append({
            "major_um2": int(best3[0]),
            "major": [int(xs[ma]), int(ys[ma]), int(zs[ma]), int(xs[mb]), int(ys[mb]), int(zs[mb])],
            "axial_z": int(zs[aa]),
            "axial_um2": int(best2[0]),
            "axial": [int(xs[aa]), int(ys[aa]), int(xs[ab]), int(ys[ab])],
            "axial_perp_extent": int(proj.max() - proj.min()),
            "axial_perp": [int(px[c]), int(py[c]), int(px[e]), int(py[e])],
        })
    return out


def measure_intensity(dilated, raw, pixel_type="u16", stored_bits=16):
    """The intensity record (nm03/measure.h IntensityStats) of one mask of any rank (torch or NumPy) in
    NumPy: the stored samples under the mask sorted, raw_pP = sorted[k − 1] with the integer nearest rank
    k = (p · n + 99) // 100 (not np.percentile: its float rank disagrees at exact multiples), and the sum
    of squares in Python integers. Returns the dict of integers ops.measure_intensity gives."""
    import numpy as np

    def to_np(t):
        return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    m = to_np(dilated).astype(bool)
    v = to_np(raw).view(np.uint16).astype(np.int64)
    sh = 16 - int(stored_bits)
    if pixel_type == "i16":
        v = ((v << sh) & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64) >> sh
    else:
        v = v & (0xFFFF >> sh)
    s = np.sort(v[m])
    n = int(s.size)
    out = {"count": n, "raw_sum_sq": sum(int(x) * int(x) for x in s)}
    for p in (10, 25, 50, 75, 90):
        out[f"raw_p{p}"] = int(s[(p * n + 99) // 100 - 1]) if n else 0
    return out


def measure_volume_intensity(dilated, raw, pixel_type="u16", stored_bits=16):
    """measure_intensity of a volume mask [D, H, W]: the same definition over the voxels."""
    return measure_intensity(dilated, raw, pixel_type, stored_bits)


GLCM_DIRECTIONS_2D = ((1, 0), (1, 1), (0, 1), (-1, 1))
GLCM_DIRECTIONS_3D = tuple((dx, dy, dz) for dz in (0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                           if dz == 1 or (dy == 1) or (dy == 0 and dx == 1))


def glcm(mask, raw, levels=32, pixel_type="u16", stored_bits=16, directions=None):
    """The grey-level co-occurrence record (nm03/texture_core.h) of one mask [H, W] or [D, H, W] (torch or
    NumPy) in NumPy: the stored samples become keys (signed data with the sign bit flipped), the keys
    levels by min(levels − 1, (key − lo) · levels // (hi − lo)), and for every direction the mask and the
    levels are compared with themselves shifted by it and the pairs scattered with np.add.at — into
    C[a, b] and C[b, a]. `directions`: (dx, dy) or (dx, dy, dz) tuples; None gives the merged forward set
    (4 in 2D, 13 in 3D). Returns the dict ops.measure_texture gives."""
    import numpy as np

    def to_np(t):
        return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    m = to_np(mask).astype(bool)
    v = to_np(raw).view(np.uint16).astype(np.int64)
    sh = 16 - int(stored_bits)
    if pixel_type == "i16":
        v = ((v << sh) & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64) >> sh
        key = (v & 0xFFFF) ^ 0x8000
    else:
        key = v & (0xFFFF >> sh)
    two_d = m.ndim == 2
    if two_d:
        m, key = m[None], key[None]
    if directions is None:
        directions = GLCM_DIRECTIONS_2D if two_d else GLCM_DIRECTIONS_3D
    ng = int(levels)
    c = np.zeros((ng, ng), np.int64)
    out = {"levels": ng, "key_lo": 0, "key_hi": 0, "samples": int(m.sum()), "pairs": 0}
    if out["samples"]:
        lo, hi = int(key[m].min()), int(key[m].max())
        out["key_lo"], out["key_hi"] = lo, hi
        lev = np.zeros_like(key) if hi == lo else np.minimum(ng - 1, (key - lo) * ng // (hi - lo))
        D, H, W = m.shape

        def window(n, s):  # the indices i with 0 <= i and i + s in [0, n), and their partners
            return (slice(max(0, -s), n - max(0, s)), slice(max(0, s), n - max(0, -s)))

        for t in directions:
            dx, dy, dz = (tuple(t) + (0,))[:3]
            (z0, z1), (y0, y1), (x0, x1) = window(D, dz), window(H, dy), window(W, dx)
            both = m[z0, y0, x0] & m[z1, y1, x1]
            a, b = lev[z0, y0, x0][both], lev[z1, y1, x1][both]
            np.add.at(c, (a, b), 1)
            np.add.at(c, (b, a), 1)
            out["pairs"] += int(both.sum())
    out["glcm"] = c.astype(np.uint32)
    return out


def glcm_features(c):
    """The 7 integers and 16 doubles the sidecar derives from a co-occurrence matrix (measure::glcm_features),
    in vectorised float64, under their sidecar keys; None where the text says null."""
    import numpy as np
    c = np.asarray(c).astype(np.int64)
    ng = c.shape[0]
    i, j = np.meshgrid(np.arange(1, ng + 1), np.arange(1, ng + 1), indexing="ij")
    d = np.abs(i - j)
    total = int(c.sum())
    out = {"glcm_levels": ng, "glcm_pairs": total // 2, "glcm_nonzero": int((c > 0).sum()), "glcm_max_count": int(c.max()),
           "glcm_sum_abs_d": int((d * c).sum()), "glcm_sum_d2": int((d * d * c).sum()),
           "glcm_sum_sq": sum(int(x) * int(x) for x in c.ravel())}
    names = ("joint_max", "joint_avg", "joint_var", "joint_entropy", "asm", "contrast", "dissimilarity", "inv_diff",
             "inv_diff_moment", "correlation", "autocorrelation", "cluster_tendency", "cluster_shade", "cluster_prominence",
             "sum_entropy", "diff_entropy")
    if total == 0:
        out.update({"glcm_" + k: None for k in names})
        return out
    p = c.astype(np.float64) / float(total)

    def entropy(q):
        q = q[q > 0]
        return float(-(q * np.log2(q)).sum())

    mu = float((i * p).sum())
    var = float(((i - mu) ** 2 * p).sum())
    s = i + j - 2 * mu
    psum = np.bincount((i + j).ravel(), weights=p.ravel())
    pdiff = np.bincount(d.ravel(), weights=p.ravel())
    vals = (float(p.max()), mu, var, entropy(p.ravel()), float((p * p).sum()), float((d * d * p).sum()), float((d * p).sum()),
            float((p / (1 + d)).sum()), float((p / (1 + d * d)).sum()),
            float(((i - mu) * (j - mu) * p).sum()) / var if var > 0 else None, float((i * j * p).sum()),
            float((s ** 2 * p).sum()), float((s ** 3 * p).sum()), float((s ** 4 * p).sum()), entropy(psum), entropy(pdiff))
    out.update({"glcm_" + k: v for k, v in zip(names, vals)})
    return out


def psnr(a, b):
    mse = ((a.double() - b.double()) ** 2).mean().item()
    return math.inf if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def volume_views(raw, dilated, at="mask", pixel_type="u16", stored_bits=16, inverted=False):
    """The dict ops.volume_views gives, in plain NumPy: slicing for the three planes, max(axis=…) (min when
    `inverted`) on the order-preserving keys for the projections, any(axis=…) for the shadows. The key of a
    sample is its value masked to `stored_bits` (sign-extended, then the sign bit flipped, for i16); a
    projection pixel is the canonical sample of the winning key (the key itself, or the sign-extended value)."""
    import numpy as np

    x = raw.detach().cpu().numpy() if isinstance(raw, torch.Tensor) else np.asarray(raw)
    x = np.ascontiguousarray(x).view(np.uint16) if x.dtype == np.int16 else x.astype(np.uint16)
    m = (dilated.detach().cpu().numpy() if isinstance(dilated, torch.Tensor) else np.asarray(dilated)).astype(bool)
    if x.ndim != 3 or m.shape != x.shape:
        raise ValueError("raw and dilated must be [D, H, W] of one shape")
    d, h, w = x.shape
    bits = int(stored_bits)
    sh = 16 - bits
    if pixel_type == "i16":
        value = ((x.astype(np.int32) << sh) & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int32) >> sh
        key = value + 32768
    else:
        value = x.astype(np.int32) & (0xFFFF >> sh)
        key = value

    def sample(k):  # the canonical stored sample of a key
        v = k - 32768 if pixel_type == "i16" else k
        return (v & 0xFFFF).astype(np.uint16)

    if m.any():
        zs, ys, xs = np.nonzero(m)
        box = [int(xs.min()), int(ys.min()), int(zs.min()), int(xs.max()), int(ys.max()), int(zs.max())]
    else:
        box = None
    if isinstance(at, str):
        if at not in ("mask", "centre"):
            raise ValueError("at must be 'mask', 'centre' or (x, y, z)")
        mode = at
        if at == "mask" and box is not None:
            p = ((box[0] + box[3]) // 2, (box[1] + box[4]) // 2, (box[2] + box[5]) // 2)
        else:
            p = (w // 2, h // 2, d // 2)
    else:
        mode = "point"
        p = tuple(int(v) for v in at)
        if len(p) != 3 or not (0 <= p[0] < w and 0 <= p[1] < h and 0 <= p[2] < d):
            raise ValueError(f"the point {p} lies outside the volume of {w} x {h} x {d}")
    best = np.min if inverted else np.max
    planes = {
        "view_axial": (x[p[2]], m[p[2]]),
        "view_coronal": (x[:, p[1], :], m[:, p[1], :]),
        "view_sagittal": (x[:, :, p[0]], m[:, :, p[0]]),
        "mip_axial": (sample(best(key, axis=0)), m.any(axis=0)),
        "mip_coronal": (sample(best(key, axis=1)), m.any(axis=1)),
        "mip_sagittal": (sample(best(key, axis=2)), m.any(axis=2)),
    }
    views = {}
    for name, (r, k) in planes.items():
        r = np.ascontiguousarray(r, dtype=np.uint16)
        if pixel_type == "i16":
            v = ((r.astype(np.int32) << sh) & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int32) >> sh
        else:
            v = r.astype(np.int32) & (0xFFFF >> sh)
        views[name] = {"width": int(r.shape[1]), "height": int(r.shape[0]), "raw": r,
                       "mask": np.ascontiguousarray(k, dtype=np.uint8), "raw_min": int(v.min()), "raw_max": int(v.max()),
                       "mask_px": int(k.sum())}
    return {"width": w, "height": h, "depth": d, "at_mode": mode, "at": p, "mask_bbox": box, "inverted": bool(inverted),
            "views": views}


def volume_mesh(mask, spacing=(1, 1, 1), placement="corner"):
    """NumPy reference of ops.volume_mesh / native.golden_volume_mesh (nm03/volume_mesh.h) on a [D, H, W] mask
    (array or CPU tensor): the same dict of vertices (float32 [V, 3]), quads (int32 [Q, 4]), quads_x / _y / _z
    and voxels, from whole-array operations on the padded mask rather than loops or word arithmetic."""
    import numpy as np
    m = np.asarray(mask.cpu() if hasattr(mask, "cpu") else mask).astype(bool)
    if m.ndim != 3:
        raise ValueError("mask must be [D, H, W]")
    if placement not in ("corner", "nets"):
        raise ValueError("placement must be 'corner' or 'nets'")
    d, h, w = m.shape
    p = np.zeros((d + 2, h + 2, w + 2), dtype=np.int8)  # voxel (x, y, z) at p[z + 1, y + 1, x + 1]
    p[1:-1, 1:-1, 1:-1] = m

    def win(dx, dy, dz):  # voxel (i - 1 + dx, j - 1 + dy, k - 1 + dz) of every corner, [d + 1, h + 1, w + 1]
        return p[dz:dz + d + 1, dy:dy + h + 1, dx:dx + w + 1]

    vox = [[[win(dx, dy, dz) for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]  # vox[dz][dy][dx]
    total = sum(vox[dz][dy][dx].astype(np.int32) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
    mixed = (total > 0) & (total < 8)
    rank = np.full(mixed.shape, -1, dtype=np.int64)
    rank[mixed] = np.arange(int(mixed.sum()))
    kk, jj, ii = np.nonzero(mixed)  # raster order (k, j, i)
    c = np.stack([ii, jj, kk], axis=1).astype(np.int64)
    if placement == "corner":
        n = np.ones(len(c), dtype=np.int64)
        s = np.zeros((len(c), 3), dtype=np.int64)
    else:
        n = np.zeros(mixed.shape, dtype=np.int64)
        s = np.zeros(mixed.shape + (3,), dtype=np.int64)
        for a in range(3):  # edges along axis a: the two voxels differ in offset a only
            for u in (0, 1):
                for v in (0, 1):
                    o0, o1 = [0, 0, 0], [0, 0, 0]
                    b, cc = (a + 1) % 3, (a + 2) % 3
                    o0[a], o1[a] = 0, 1
                    o0[b] = o1[b] = u
                    o0[cc] = o1[cc] = v
                    cross = vox[o0[2]][o0[1]][o0[0]] != vox[o1[2]][o1[1]][o1[0]]
                    n += cross
                    s[..., b] += cross * (2 * u - 1)
                    s[..., cc] += cross * (2 * v - 1)
        n = n[mixed]
        s = s[mixed]
    num = (2 * c - 1) * n[:, None] + s
    sp = np.asarray([np.float32(spacing[0]), np.float32(spacing[1]), np.float32(np.float64(spacing[2]))], dtype=np.float32)
    verts = (num.astype(np.float32) / (2 * n[:, None]).astype(np.float32)).astype(np.float32) * sp[None, :]
    verts = verts.astype(np.float32).reshape(-1, 3)
    quads, counts = [], []
    e = np.eye(3, dtype=np.int64)
    for a in range(3):
        b, cc = (a + 1) % 3, (a + 2) % 3
        sl_lo = [slice(1, -1)] * 3  # numpy axes are (z, y, x): axis a of the mesh is numpy axis 2 - a
        sl_hi = [slice(1, -1)] * 3
        sl_lo[2 - a] = slice(0, -1)
        sl_hi[2 - a] = slice(1, None)
        lower, upper = p[tuple(sl_lo)], p[tuple(sl_hi)]  # voxel p - e_a and voxel p for p_a in [0, dim_a]
        pz, py, px = np.nonzero(lower != upper)
        pos = np.stack([px, py, pz], axis=1).astype(np.int64)
        low_set = lower[pz, py, px] == 1
        cs = [pos, pos + e[b], pos + e[b] + e[cc], pos + e[cc]]
        idx = [rank[q[:, 2], q[:, 1], q[:, 0]] for q in cs]
        q = np.stack([idx[0], np.where(low_set, idx[1], idx[3]), idx[2], np.where(low_set, idx[3], idx[1])], axis=1)
        quads.append(q)
        counts.append(len(q))
    quads = np.concatenate(quads, axis=0).astype(np.int32).reshape(-1, 4)
    return {"width": w, "height": h, "depth": d, "placement": placement, "vertices": verts, "quads": quads,
            "quads_x": counts[0], "quads_y": counts[1], "quads_z": counts[2], "voxels": int(m.sum())}


NO_DISTANCE = 2 ** 63 - 1


def _distance_set(mask, to):
    import numpy as np
    m = np.asarray(mask.cpu() if hasattr(mask, "cpu") else mask).astype(bool)
    if m.ndim != 3:
        raise ValueError("mask must be [D, H, W]")
    if to not in ("foreground", "background"):
        raise ValueError("to must be 'foreground' or 'background'")
    return m if to == "foreground" else ~m


def _apply_cap(dist, cap_um):
    if cap_um is not None:
        if int(cap_um) < 0:
            raise ValueError("cap_um must not be negative")
        dist[dist > int(cap_um) ** 2] = NO_DISTANCE
    return dist


def volume_distance(mask, spacing_um=(1000, 1000, 1000), to="foreground", cap_um=None):
    """Reference of ops.volume_distance / native.golden_volume_distance (nm03/volume_distance.h) on a [D, H, W]
    mask (array or CPU tensor) → int64 array [D, H, W]. SciPy's distance_transform_edt names a nearest voxel of S
    for every voxel (return_indices, sampling = (uz, uy, ux)); the squared distance is then RECOMPUTED IN INT64
    from those indices, so no float of SciPy's is ever compared. Outside the frame is neither S nor its
    complement, which is SciPy's own convention."""
    import numpy as np
    from scipy import ndimage
    s = _distance_set(mask, to)
    ux, uy, uz = (int(v) for v in spacing_um)
    if not s.any():
        return np.full(s.shape, NO_DISTANCE, dtype=np.int64)
    idx = ndimage.distance_transform_edt(~s, sampling=(float(uz), float(uy), float(ux)), return_distances=False,
                                         return_indices=True)
    zz, yy, xx = np.indices(s.shape)
    dz = (zz - idx[0]).astype(np.int64) * uz
    dy = (yy - idx[1]).astype(np.int64) * uy
    dx = (xx - idx[2]).astype(np.int64) * ux
    return _apply_cap(dx * dx + dy * dy + dz * dz, cap_um)


def volume_distance_brute(mask, spacing_um=(1000, 1000, 1000), to="foreground", cap_um=None):
    """The same map by all pairs in int64 (NumPy broadcasting): for the tiny cases."""
    import numpy as np
    s = _distance_set(mask, to)
    ux, uy, uz = (int(v) for v in spacing_um)
    if not s.any():
        return np.full(s.shape, NO_DISTANCE, dtype=np.int64)
    qz, qy, qx = (a.astype(np.int64) for a in np.nonzero(s))
    zz, yy, xx = (a.reshape(-1, 1).astype(np.int64) for a in np.indices(s.shape))
    d2 = ((xx - qx) * ux) ** 2 + ((yy - qy) * uy) ** 2 + ((zz - qz) * uz) ** 2
    return _apply_cap(d2.min(axis=1).reshape(s.shape), cap_um)


def dilate_volume_mm(mask, spacing_um=(1000, 1000, 1000), radius_um=0):
    """Reference of ops.dilate_volume_mm: the threshold D_mask ≤ radius_um² of the reference map → bool array."""
    if int(radius_um) < 0:
        raise ValueError("radius_um must not be negative")
    return volume_distance(mask, spacing_um, "foreground") <= int(radius_um) ** 2


def volume_thickness(mask, spacing_um=(1000, 1000, 1000)):
    """Reference of ops.volume_thickness: the largest background distance over the mask voxels, the first voxel
    in raster (z, y, x) order that attains it, and the two derived lengths."""
    import numpy as np
    m = _distance_set(mask, "foreground")
    dist = volume_distance(m, spacing_um, "background")
    cand = m & (dist != NO_DISTANCE)
    if not cand.any():
        return {"inscribed_um2": 0, "inscribed_at": [-1, -1, -1], "found": False, "inscribed_radius_mm": None,
                "thickness_mm": None}
    v = np.where(cand, dist, -1)
    best = int(v.max())
    z, y, x = (int(a) for a in np.unravel_index(int(np.argmax(v)), v.shape))  # argmax: the first in raster order
    r = math.sqrt(float(best)) / 1000.0
    return {"inscribed_um2": best, "inscribed_at": [x, y, z], "found": True, "inscribed_radius_mm": r, "thickness_mm": 2.0 * r}


def volume_surface(mask):
    """S(M) of nm03/volume_compare.h: the voxels of M with an open 6-face, outside the frame counting as open —
    M ^ binary_erosion(M, generate_binary_structure(3, 1)) → bool array."""
    from scipy import ndimage
    m = _distance_set(mask, "foreground")
    return m ^ ndimage.binary_erosion(m, ndimage.generate_binary_structure(3, 1))


def _compare_directed(s_from, s_to, spacing_um, tag, out):
    import numpy as np
    found = bool(s_from.any() and s_to.any())
    out["found" + tag] = found
    if not found:
        out.update({"n" + tag: 0, "max_um2" + tag: 0, "worst" + tag: [-1, -1, -1], "sum_um" + tag: 0, "p95_um" + tag: 0})
        return
    dist = volume_distance(s_to, spacing_um, "foreground")  # SciPy for indices only; d² recomputed in int64
    dv = dist[s_from]  # raster order
    keys = np.sort(np.array([math.isqrt(int(v)) for v in dv], dtype=np.int64))
    n = int(keys.size)
    first = int(np.argmax(dv))  # the first in raster order at the maximum
    z, y, x = (int(c[first]) for c in np.nonzero(s_from))
    out.update({"n" + tag: n, "max_um2" + tag: int(dv.max()), "worst" + tag: [x, y, z], "sum_um" + tag: int(keys.sum()),
                "p95_um" + tag: int(keys[(95 * n + 99) // 100 - 1])})


def compare_volumes(a, b, spacing_um=(1000, 1000, 1000)):
    """Reference of ops.compare_volumes / native.golden_compare_volumes on two [D, H, W] masks (arrays or CPU
    tensors) → the same dict of integers. SciPy's erosion gives the surfaces; distance_transform_edt is used for
    indices only (volume_distance above recomputes d² in int64, no float of SciPy's is compared); math.isqrt and
    np.sort do the rest."""
    import numpy as np
    ma, mb = _distance_set(a, "foreground"), _distance_set(b, "foreground")
    if ma.shape != mb.shape:
        raise ValueError("both masks must be [D, H, W] of one shape")
    tp = int((ma & mb).sum())
    out = {"a_vox": int(ma.sum()), "b_vox": int(mb.sum()), "tp_vox": tp, "fp_vox": int(ma.sum()) - tp, "fn_vox": int(mb.sum()) - tp}
    sa, sb = volume_surface(ma), volume_surface(mb)
    out["surface_a"], out["surface_b"] = int(sa.sum()), int(sb.sum())
    _compare_directed(sa, sb, spacing_um, "_ab", out)
    _compare_directed(sb, sa, spacing_um, "_ba", out)
    return out


def _lesion_records(lab, n_lab, other_lab, order, other_order, table, is_a, n_max):
    import numpy as np
    out = []
    others = len(other_order)
    for i, l in enumerate(order):
        where = lab == l
        first = int(np.flatnonzero(where.ravel())[0])  # raster (z, y, x) order
        d, h, w = lab.shape
        line = table[i, :] if is_a else table[:, i]
        partners = np.unique(other_lab[where & (other_lab > 0)])
        best, best_o = -1, 0
        for j in range(others):
            if int(line[j]) > best_o:  # a tie keeps the smaller index
                best, best_o = j, int(line[j])
        out.append({"voxels": int(where.sum()), "first": [first % w, first // w % h, first // (w * h)], "overlap_vox": int(line.sum()),
                    "partners_reported": int((line[:others] > 0).sum()), "overlap_other_vox": int(line[n_max]),
                    "multi": int(partners.size >= 2), "best": best, "best_overlap_vox": best_o})
    return out


def compare_volume_lesions(a, b, max_lesions, connectivity=26):
    """Reference of ops.compare_volume_lesions / native.golden_compare_volume_lesions on two [D, H, W] masks (arrays
    or CPU tensors) → the same dict, `table` as an int64 array. scipy.ndimage.label with generate_binary_structure(3, 1)
    or (3, 3) gives the components (its labels are in the order of the first voxels), np.add.at on the label pairs of
    A ∩ B the table, np.unique of the pairs the partners."""
    import numpy as np
    from scipy import ndimage
    ma, mb = _distance_set(a, "foreground"), _distance_set(b, "foreground")
    if ma.shape != mb.shape:
        raise ValueError("both masks must be [D, H, W] of one shape")
    n = int(max_lesions)
    if not 1 <= n <= 64:
        raise ValueError("max_lesions must be 1..64")
    if connectivity not in (6, 26):
        raise ValueError("connectivity must be 6 or 26")
    st = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    la, na = ndimage.label(ma, structure=st)
    lb, nb = ndimage.label(mb, structure=st)
    both = ma & mb
    pairs = np.unique(np.stack([la[both], lb[both]], axis=1), axis=0) if both.any() else np.zeros((0, 2), dtype=np.int64)
    out = {"connectivity": int(connectivity), "max_lesions": n, "lesions_a": int(na), "lesions_b": int(nb)}
    for tag, col in (("a", 0), ("b", 1)):
        ids, cnt = np.unique(pairs[:, col], return_counts=True)
        out["hit_" + tag] = int(ids.size)
        out["multi_" + tag] = int((cnt >= 2).sum())

    def order(lab, count):  # labels: more voxels first, then the earlier first voxel (= the smaller label)
        sizes = np.bincount(lab.ravel(), minlength=count + 1)[1:]
        return [int(i) + 1 for i in np.lexsort((np.arange(count), -sizes))][:n]

    oa, ob = order(la, na), order(lb, nb)
    rank_a = np.full(na + 1, n, dtype=np.int64)
    rank_b = np.full(nb + 1, n, dtype=np.int64)
    rank_a[oa] = np.arange(len(oa))
    rank_b[ob] = np.arange(len(ob))
    table = np.zeros((n + 1, n + 1), dtype=np.int64)
    np.add.at(table, (rank_a[la[both]], rank_b[lb[both]]), 1)
    out["a_lesions"] = _lesion_records(la, na, lb, oa, ob, table, True, n)
    out["b_lesions"] = _lesion_records(lb, nb, la, ob, oa, table, False, n)
    out["table"] = table
    return out
