"""The numpy statement of the map vectorisation ("Map vectorisation"; the device form is K13,
nautilus_amd/csrc/nhip_vectorize.hip), and the crafted inputs its tests share.  Written differently from the kernels on
purpose: the votes are counted from scratch every round with np.bincount, the peak is np.argmax, the band's bins come from
np.unique and the runs from an explicit loop; no code is shared with the product.

A spec is anything with the fields of nhip_vectorize_spec_t as attributes (a ctypes struct, or make_spec() below).

PERTURB names the four deliberate mistakes the tests use to show that the crafted cases discriminate:
  "tie_largest"   equal votes go to the LARGEST index
  "band_plus_one" the band's half width is one unit of 2^-14 cell wider
  "gap_le"        neighbours of a run differ by at most max_gap (instead of max_gap + 1)
  "retire_late"   retired cells lose their votes but can still fall into a band for one more round (a kernel that subtracts
                  the votes and forgets the live byte; cells that kept their votes too would only be retired twice and
                  change no record)
"""
import math
from types import SimpleNamespace

import numpy as np

Q = 14
FIELDS = ("res", "band", "cell_x0", "cell_y0", "width", "height", "min_hits", "n_theta", "min_votes", "max_gap", "min_length",
          "max_segments", "flags", "reserved")
PERTURB = ("tie_largest", "band_plus_one", "gap_le", "retire_late")


def make_spec(**kw):
    s = SimpleNamespace(res=0.05, band=1.5, cell_x0=0, cell_y0=0, width=1, height=1, min_hits=2, n_theta=360, min_votes=20,
                        max_gap=4, min_length=10, max_segments=4096, flags=0, reserved=0)
    for k, v in kw.items():
        assert k in FIELDS, k
        setattr(s, k, v)
    return s


def pose_affines(poses):
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(P), 4), np.float32)
    for i, (x, y, th) in enumerate(P):
        with np.errstate(over="ignore"):
            out[i] = (np.float32(math.cos(th)), np.float32(math.sin(th)), np.float32(x), np.float32(y))
    return out


def world_points(xy, offsets, affines):
    """float32 (n, 2): every point of every scan that is a scan (first offset >= 0, end >= start), transformed."""
    f = np.float32
    xy = np.asarray(xy, dtype=f).reshape(-1, 2)
    off = np.asarray(offsets, dtype=np.int64)
    parts = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(off) - 1):
            if off[i] < 0 or off[i + 1] < off[i]:
                continue
            p = xy[off[i]:off[i + 1]]
            c, s, tx, ty = (f(v) for v in affines[i])
            x = ((c * p[:, 0]).astype(f) + ((-s) * p[:, 1]).astype(f)).astype(f) + tx
            y = ((s * p[:, 0]).astype(f) + (c * p[:, 1]).astype(f)).astype(f) + ty
            parts.append(np.stack([x.astype(f), y.astype(f)], axis=1))
    return np.concatenate(parts).astype(f) if parts else np.zeros((0, 2), f)


def raster(points, spec):
    """counts int32 (height, width)"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    p = p[np.isfinite(p).all(axis=1)]
    with np.errstate(over="ignore"):
        fx, fy = np.floor(p[:, 0] / spec.res), np.floor(p[:, 1] / spec.res)
    # (integer-valued doubles against small integers: exact; a floor beyond int64 is beyond the window too)
    ok = (fx >= spec.cell_x0) & (fx < spec.cell_x0 + spec.width) & (fy >= spec.cell_y0) & (fy < spec.cell_y0 + spec.height)
    cx = fx[ok].astype(np.int64) - spec.cell_x0
    cy = fy[ok].astype(np.int64) - spec.cell_y0
    return np.bincount(cy * spec.width + cx, minlength=spec.width * spec.height).reshape(spec.height, spec.width).astype(np.int32)


def cell_list(counts, min_hits):
    cy, cx = np.nonzero(counts >= min_hits)  # (row-major: cy, then cx)
    return np.stack([cx, cy], axis=1).astype(np.int32)


def tables(n_theta):
    C = np.array([int(np.rint(16384.0 * math.cos(math.pi * t / n_theta))) for t in range(n_theta)], dtype=np.int32)
    S = np.array([int(np.rint(16384.0 * math.sin(math.pi * t / n_theta))) for t in range(n_theta)], dtype=np.int32)
    return C, S


def hough(cells, spec, max_rounds=None, perturb=None):
    """(records int64 (n, 10), stats int32 (8,), initial votes int32 (n_theta, n_rho), live bool (M,))"""
    assert perturb is None or perturb in PERTURB
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    M, w, h, nt = len(cells), spec.width, spec.height, spec.n_theta
    n_rho = 2 * w + h + 1
    cx, cy = cells[:, 0], cells[:, 1]
    C, S = (v.astype(np.int64) for v in tables(nt))
    rho_all = cx[None, :] * C[:, None] + cy[None, :] * S[:, None] + (w << Q)
    assert M == 0 or (rho_all.min() >= 0 and rho_all.max() < 2 ** 31)
    flat = (rho_all >> Q) + np.arange(nt)[:, None] * n_rho
    band_q = int(np.rint(spec.band * 16384.0)) + (perturb == "band_plus_one")
    step = spec.max_gap + (0 if perturb == "gap_le" else 1)
    live = np.ones(M, dtype=bool)
    ghosts = np.zeros(M, dtype=bool)  # "retire_late" only
    count = lambda: np.bincount(flat[:, live].ravel(), minlength=nt * n_rho)
    votes0 = count().reshape(nt, n_rho).astype(np.int32)
    records, rounds, emitted, retired, flag = [], 0, 0, 0, 0
    while True:
        v = count()
        idx = len(v) - 1 - int(np.argmax(v[::-1])) if perturb == "tie_largest" else int(np.argmax(v))
        if v[idx] < spec.min_votes:
            flag = 0
            break
        if max_rounds is not None and rounds >= max_rounds:
            flag = 1
            break
        t, b = divmod(idx, n_rho)
        rho = cx * C[t] + cy * S[t] + (w << Q)
        a = (cy * C[t] - cx * S[t] + (w << Q)) >> Q  # (numpy's >> on negative int64 is the floor)
        band = (live | ghosts) & (np.abs(rho - ((b << Q) + (1 << (Q - 1)))) <= band_q)
        ghosts[:] = False
        bins = np.unique(a[band])
        runs, lo, prev = [], int(bins[0]), int(bins[0])
        for x in bins[1:]:
            x = int(x)
            if x - prev > step:
                runs.append((lo, prev))
                lo = x
            prev = x
        runs.append((lo, prev))
        kept = [r for r in runs if r[1] - r[0] + 1 >= spec.min_length]
        if not kept:
            retired += int((band & live).sum())
            if perturb == "retire_late":
                ghosts = band.copy()
            live &= ~band
        elif len(records) + len(kept) > spec.max_segments:
            flag = 2
            break
        else:
            for lo, hi in kept:
                sel = band & (a >= lo) & (a <= hi)
                x, y = cx[sel], cy[sel]
                records.append([t, b, lo, hi, int(sel.sum()), int(x.sum()), int(y.sum()), int((x * x).sum()), int((x * y).sum()),
                                int((y * y).sum())])
                emitted += int((sel & live).sum())
                live &= ~sel
        rounds += 1
    stats = np.array([M, len(records), rounds, flag, emitted, retired, n_rho, 0], dtype=np.int32)
    return np.array(records, dtype=np.int64).reshape(-1, 10), stats, votes0, live


def endpoints(spec, records):
    """float32 (n, 4): the numpy counterpart of nhip_vectorize_endpoints; python floats (doubles) and libm through math"""
    C, S = tables(spec.n_theta)
    out = np.zeros((len(records), 4), np.float32)
    for i, r in enumerate(np.asarray(records, dtype=np.int64).reshape(-1, 10)):
        t, b, a_lo, a_hi, n, sx, sy, sxx, sxy, syy = (int(v) for v in r)
        n, sx, sy = float(n), float(sx), float(sy)
        mx, my = sx / n, sy / n
        cxx, cxy, cyy = float(sxx) - sx * mx, float(sxy) - sx * my, float(syy) - sy * my
        phi = 0.5 * math.atan2(2.0 * cxy, cxx - cyy)
        dx, dy = math.cos(phi), math.sin(phi)
        c, s = float(C[t]) / 16384.0, float(S[t]) / 16384.0
        rho = float((b << Q) + (1 << (Q - 1)) - (spec.width << Q)) / 16384.0
        for e, a in enumerate((a_lo, a_hi + 1)):
            alpha = float(a - spec.width)
            px, py = rho * c - alpha * s, rho * s + alpha * c
            u = (px - mx) * dx + (py - my) * dy
            qx, qy = mx + u * dx, my + u * dy
            out[i, 2 * e] = np.float32(((float(spec.cell_x0) + qx) + 0.5) * spec.res)
            out[i, 2 * e + 1] = np.float32(((float(spec.cell_y0) + qy) + 0.5) * spec.res)
    return out


def vectorize(xy, offsets, poses, spec, max_rounds=None, max_cells=None, perturb=None):
    """The whole step: dict(counts, cells, votes (initial), records, stats, lines, live)."""
    counts = raster(world_points(xy, offsets, pose_affines(poses)), spec)
    cells = cell_list(counts, spec.min_hits)
    if max_cells is not None and len(cells) > max_cells:
        stats = np.array([len(cells), 0, 0, 3, 0, 0, 2 * spec.width + spec.height + 1, 0], dtype=np.int32)
        return dict(counts=counts, cells=cells, votes=None, records=np.zeros((0, 10), np.int64), stats=stats,
                    lines=np.zeros((0, 4), np.float32), live=None)
    records, stats, votes, live = hough(cells, spec, max_rounds, perturb)
    return dict(counts=counts, cells=cells, votes=votes, records=records, stats=stats, lines=endpoints(spec, records), live=live)


# ---------------------------------------------------------------- crafted inputs
def scan_of_cells(cells, spec, hits=None):
    """One scan (identity pose) with `hits` points (default: min_hits) at the centre of every cell (cx, cy) of the window."""
    hits = spec.min_hits if hits is None else hits
    c = np.asarray(cells, dtype=np.float64).reshape(-1, 2)
    pts = np.stack([(c[:, 0] + spec.cell_x0 + 0.5) * spec.res, (c[:, 1] + spec.cell_y0 + 0.5) * spec.res], axis=1)
    xy = np.repeat(pts, hits, axis=0).astype(np.float32)
    return xy, np.array([0, len(xy)], dtype=np.int32), np.zeros((1, 3))


def hline(y, x0, x1, step=1):
    return [(x, y) for x in range(x0, x1 + 1, step)]


def vline(x, y0, y1):
    return [(x, y) for y in range(y0, y1 + 1)]


def crafted():
    """name -> (cells, spec): small windows, n_theta 4 (0, 45, 90, 135 degrees) unless the case is about something else,
    min_hits 1, min_votes 3."""
    base = dict(width=96, height=64, min_hits=1, n_theta=4, min_votes=3, min_length=10, max_gap=4)
    out = {}
    out["one_line"] = (hline(20, 10, 39), make_spec(**base))
    # two lines with equal votes: the smaller index (the vertical one, t = 0) wins the first round
    out["tie"] = (hline(40, 50, 69) + vline(20, 5, 24), make_spec(**base))
    # a cross: the shared cell goes to the first line
    out["cross"] = (hline(30, 20, 60) + vline(40, 10, 50), make_spec(**base))
    # a dotted line: gaps of exactly max_gap (bridged) and max_gap + 1 (a new run)
    dotted = hline(12, 5, 16) + hline(12, 21, 32) + hline(12, 38, 49)
    out["dotted"] = (dotted, make_spec(**base))
    # runs of min_length - 1 (dropped: retires) and min_length (kept)
    out["lengths"] = (hline(8, 3, 11) + hline(50, 3, 12), make_spec(**base))
    # a cell at exactly the band's half width from the peak bin's centre: rows y, y + 1 ... of a thick line
    out["thick"] = (hline(20, 10, 39) + hline(22, 10, 39, 3) + hline(19, 10, 39, 2), make_spec(**base))
    # the same cells under a band one unit narrower than 1.5 cells: the rows at exactly 1.5 cells from the centre stay out
    out["band_edge"] = (out["thick"][0], make_spec(**dict(base, band=1.5 - 2.0 ** -14)))
    # a line whose normal points at 135 degrees (C < 0): along-line bins on both sides of 0
    out["diag_neg"] = ([(x, x - 40) for x in range(56, 96)], make_spec(**base))
    # a blob that only retires
    out["blob"] = ([(x, y) for x in range(30, 34) for y in range(30, 35)], make_spec(**base))
    # a stub that retires beside a short line that on its own retires too: cells retired late would join it
    stub = vline(5, 12, 19) + vline(6, 12, 19) + hline(15, 8, 13) + hline(40, 0, 29)
    out["stub"] = (stub, make_spec(**dict(base, min_length=9)))
    return out
