#!/usr/bin/env python3
"""Localise scans in a finished map, through the map files.

The first --map-scans scans of a synthetic bag are mapped at their truth poses (or at the poses a growing-window solve gives
them): the occupancy grid is ray-traced, written as STEM.pgm / STEM.yaml (map_server's pair, hostside.write_occupancy_map) and
read back.  Every remaining scan is then localised in that map from its odometry pose -- the last mapped scan's pose carried on
by the odometry increments, drift included: the occupied cells around the prior become the matcher's target (DESIGN.md
section 3, "Map windows") and the best pose of the lattice is the answer.  Prints one JSON line: queries, rejected, position
and heading errors against the truth, points per window.

  --no-prior        the same run with the odometry priors replaced by global localisation ("Range
                    signatures"): K proposals per scan from the range signatures of the map alone, every one of them matched,
                    the best-scoring one kept.  The JSON line gains the winning ranks.

  --backend hip     the product: HipBackend.occupancy_grid and HipBackend.localize, everything on the GPU
  --backend oracle  no device: the numpy statement of the occupancy grid the tests keep, hostside.localize (windows in numpy)
                    and the CPU oracle's matcher
"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nautilus_amd import csm, hostside, synth  # noqa: E402


def relative(a, b):
    """b in a's frame: (x, y, theta) each"""
    c, s = math.cos(a[2]), math.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, b[2] - a[2]])


def compose(pose, rel):
    c, s = math.cos(pose[2]), math.sin(pose[2])
    return np.array([pose[0] + c * rel[0] - s * rel[1], pose[1] + s * rel[0] + c * rel[1], pose[2] + rel[2]])


def run(n_scans=120, n_map=80, backend="hip", map_poses="truth", stem="localize_map", min_score=None, device="cuda:0", every=1,
        no_prior=False):
    bag = synth.SynthBag(n_scans)
    if not 0 < n_map < n_scans:
        raise ValueError("run: %d of %d scans for the map" % (n_map, n_scans))
    if backend == "hip":
        from nautilus_amd import occupancy, posegraph
        be = posegraph.HipBackend(device)
    else:
        from oracle.cpu_backend import OracleBackend
        from tests import occupancy_reference
        be = OracleBackend()
    mxy, moff = csm.pack_scans(bag.scans[:n_map])
    if map_poses == "solved":
        from nautilus_amd import posegraph
        nrm = np.concatenate(bag.normals[:n_map]).astype(np.float32)
        _, poses = posegraph.solve_growing_window(mxy, nrm, moff, bag.odom[:n_map], window_max=5, device=device, backend=be)
    else:
        poses = bag.truth[:n_map].copy()
    x0, y0, w, h = hostside.map_window(poses, 30.0, 0.05)
    if backend == "hip":
        occ = occupancy.spec(cell_x0=x0, cell_y0=y0, width=w, height=h)
        grid = be.occupancy_grid(poses, spec=occ, xy=mxy, offsets=moff)[0]
    else:
        occ = occupancy_reference.make_spec(cell_x0=x0, cell_y0=y0, width=w, height=h)
        grid = occupancy_reference.occupancy(mxy, moff, poses, occ)[0]
    hostside.write_occupancy_map(stem, grid, occ)
    # ---- from here on only the two files are known
    grid, info = hostside.read_occupancy_map(stem)
    res, cx0, cy0, width, height = hostside.occupancy_map_window(grid, info)
    window = argparse.Namespace(res=res, cell_x0=cx0, cell_y0=cy0, width=width, height=height)
    q = np.arange(n_map, n_scans, max(int(every), 1))
    priors = np.array([compose(poses[n_map - 1], relative(bag.odom[n_map - 1], bag.odom[i])) for i in q])
    qxy, qoff = csm.pack_scans([bag.scans[i] for i in q])
    if no_prior:
        r = be.global_localize(qxy, qoff, grid, window, min_score=min_score) if backend == "hip" else \
            hostside.global_localize(be, qxy, qoff, grid, window)
        won = np.maximum(r["rank"], 0)
        proposed = r["proposals"][np.arange(len(q)), won]
        priors = np.where(np.isnan(proposed), priors, proposed)  # (what "prior_error" reports: the winning proposals)
        # (a window per proposal: the winner's points are not kept apart; the map's occupied cells stand in for them)
        r = {"poses": r["poses"], "records": r["records"][np.arange(len(q)), won], "rejected": r["rank"] < 0, "ranks": r["rank"],
             "points_per_window": np.full(len(q), int((grid == 100).sum()), np.int32)}
    elif backend == "hip":
        r = be.localize(qxy, qoff, priors, grid, window, min_score=min_score)
    else:
        r = hostside.localize(be, qxy, qoff, priors, grid, window)
    ok = ~r["rejected"]
    e = r["poses"][ok] - bag.truth[q][ok]
    pos = np.hypot(e[:, 0], e[:, 1])
    ang = np.degrees(np.abs(csm.angle_mod(e[:, 2])))
    pe = priors - bag.truth[q]
    ppw = r["points_per_window"]
    extra = {"no_prior": True, "ranks": [int(v) for v in r["ranks"]]} if no_prior else {}
    return {**extra, "backend": be.name, "n_scans": n_scans, "map_scans": n_map, "map_poses": map_poses, "map": [stem + ".pgm", stem + ".yaml"],
            "map_cells": [int(width), int(height)], "map_cells_occupied": int((grid == 100).sum()),
            "queries": int(len(q)), "rejected": int(r["rejected"].sum()),
            "prior_error_max_m": float(np.hypot(pe[:, 0], pe[:, 1]).max()),
            "prior_heading_error_max_deg": float(np.degrees(np.abs(csm.angle_mod(pe[:, 2]))).max()),
            "position_error_max_m": float(pos.max()) if len(pos) else None,
            "position_error_mean_m": float(pos.mean()) if len(pos) else None,
            "heading_error_max_deg": float(ang.max()) if len(ang) else None,
            "score_min": float(r["records"]["score"][ok].min()) if ok.any() else None,
            "points_per_window_min": int(ppw.min()), "points_per_window_max": int(ppw.max()),
            "poses": [[None if math.isnan(v) else float(v) for v in p] for p in r["poses"]]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["oracle", "hip"], default="hip")
    ap.add_argument("--scans", type=int, default=120, help="scans of the synthetic bag")
    ap.add_argument("--map-scans", type=int, default=80, help="the first scans, which make the map; the rest are localised in it")
    ap.add_argument("--map-poses", choices=["truth", "solved"], default="truth",
                    help="map the first scans at their truth poses, or at the poses of a growing-window solve from their odometry")
    ap.add_argument("--map", metavar="STEM", default="localize_map", help="writes STEM.pgm and STEM.yaml, then reads them back")
    ap.add_argument("--min-score", type=float, default=None, help="--backend hip: reject matches that score below this")
    ap.add_argument("--every", type=int, default=1, help="localise every n-th of the remaining scans")
    ap.add_argument("--no-prior", action="store_true", help="global localisation: proposals from the map's range signatures, no odometry")
    a = ap.parse_args()
    print(json.dumps(run(a.scans, a.map_scans, a.backend, a.map_poses, a.map, a.min_score, every=a.every, no_prior=a.no_prior)))
