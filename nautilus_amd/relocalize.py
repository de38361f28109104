"""Global localisation in a finished occupancy grid: scans localised from NO prior.

rangesig.py proposes K poses per scan from the map alone (kernel unit K21: range signatures of the map's free lattice cells,
matched with the scan's by byte SAD under 64 rotations); the unchanged localize.localize then matches every (scan, proposal)
entry on the device -- the scans repeated in the packed cloud -- and per query the entry with the highest record score wins,
ties to the lower rank.  hostside.global_localize is the same route in numpy for any backend with a match() method; the two
share the second half (hostside.global_localize_finish), so they differ by where the signatures, the records and the matches
are computed and by nothing else.
"""
import numpy as np

from . import hostside, localize, rangesig


def global_localize(xy, offsets, grid, occ_spec, spec=None, grid_spec=None, search=None, min_score=None, cell_bits=16, occ_min=100,
                    device="cuda:0", max_slots=128, max_anchors=None):
    """Scan q of the packed scans (xy, offsets) localised in `grid` (int8 (H, W): what occupancy_grid returned or
    read_occupancy_map read; occ_spec: its window and res) without a prior.  spec: a RangesigSpec (None: the defaults on
    occ_spec's window and res with NHIP_RANGESIG_UNKNOWN_STOPS, occ_min as given); grid_spec, search, min_score, cell_bits,
    max_slots: localize.localize's.
    Returns the dict of hostside.global_localize: poses (Q, 3) float64, NaN where no entry matched; rank int32 (Q,), the winning
    proposal, -1 likewise; proposals (Q, K, 3); candidates int32 (Q, K, 4); anchors int32 (A, 4); records MATCH_DTYPE (Q, K);
    stats int64 (8,)."""
    spec = rangesig.spec(occ_spec, occ_min=int(occ_min), flags=rangesig.NHIP_RANGESIG_UNKNOWN_STOPS) if spec is None else spec
    c = rangesig.candidates(grid, spec, xy, offsets, device=device, max_anchors=max_anchors)

    def on_device(xy2, off2, priors, grid, occ_spec, **kw):
        return localize.localize(xy2, off2, priors, grid, occ_spec, min_score=min_score, device=device, max_slots=max_slots, **kw)
    return hostside.global_localize_finish(on_device, xy, offsets, np.asarray(c["records"]), c["anchors"], spec, c["stats"], grid, occ_spec,
                                           dict(occ_min=occ_min, cell_bits=cell_bits, grid_spec=grid_spec, search=search))
