"""What the tests of the global localisation share: the mapped lap of the synthetic world, the queries without priors, and the
errors the host route leaves on them with the CPU oracle's matcher (measured by tests/test_relocalize_cpu.py)."""
import functools

import numpy as np

from nautilus_amd import csm, hostside, synth
from tests import occupancy_reference as OR

MAP_SCANS = 400
QUERIES = list(range(1, MAP_SCANS, 18))  # 23 odd scans, 1 .. 397: none of them is in the map
# hostside.global_localize with the CPU oracle's matcher on QUERIES, largest errors against the truth (measured:
# test_global_localize_on_the_cpu_oracle prints them): 0.0598 m, 0.2799 degrees
ORACLE_POSITION_ERROR_M, ORACLE_HEADING_ERROR_DEG = 0.060, 0.280


def lap():
    return synth.SynthBag(MAP_SCANS)


def map_inputs(bag):
    """(xy, offsets, poses, window) of the map: the even scans at their truth poses, the window of every pose +- 30 m"""
    even = list(range(0, MAP_SCANS, 2))
    xy, off = csm.pack_scans([bag.scans[i] for i in even])
    return xy, off, bag.truth[even], hostside.map_window(bag.truth, 30.0, 0.05)


@functools.lru_cache(maxsize=None)
def mapped_lap():
    """SynthBag(400), the map of its 200 even scans at their truth poses through tests/occupancy_reference.occupancy with the
    defaults: (bag, grid int8 (1544, 1843), occ)"""
    bag = lap()
    xy, off, poses, (x0, y0, w, h) = map_inputs(bag)
    occ = OR.make_spec(cell_x0=x0, cell_y0=y0, width=w, height=h)
    return bag, OR.occupancy(xy, off, poses, occ)[0], occ


def near_truth(proposals, truth):
    """(Q, K) bool: the proposal lies within 1 m and 15 degrees of the truth"""
    e = proposals - truth[:, None, :]
    return (np.hypot(e[..., 0], e[..., 1]) <= 1.0) & (np.degrees(np.abs(csm.angle_mod(e[..., 2]))) <= 15.0)


def errors(poses, truth):
    """(position error in metres, heading error in degrees) per query"""
    e = poses - truth
    return np.hypot(e[:, 0], e[:, 1]), np.degrees(np.abs(csm.angle_mod(e[:, 2])))
