"""The sequence form of the appearance gate inside the example loop ("Place sequences"): --lc-sequence W
proposes the same pairs on the product as on the oracle's CPU backend, W = 0 is the run without the flag, and the flag is refused
with any other gate."""
import pytest

pytestmark = pytest.mark.gpu

KW = dict(n_scans=32, window=3, spacing=0.06, hitl=False, gate="geometric", iterations=2)  # (the other loop tests' bag)


def test_the_loop_proposes_by_sequence_on_the_device_what_the_host_path_proposes(gpu):
    import examples.slam_loop as loop
    from oracle.cpu_backend import OracleBackend
    dev = loop.run(lc_gate="appearance", lc_sequence=2, **KW)
    host = loop.run(backend=OracleBackend(), lc_gate="appearance", lc_sequence=2, **KW)
    assert dev["backend"] == "hip" and dev["lc_gate"] == host["lc_gate"] == "appearance" and dev["place_s"] > 0
    assert dev["lc_pairs"] == host["lc_pairs"] and len(dev["lc_pairs"]) == dev["lc_candidates"] > 0
    for key in ("lc_sequence", "lc_sequence_step", "lc_sequence_reverse", "lc_sequence_short"):
        assert dev[key] == host[key]
    assert (dev["lc_sequence"], dev["lc_sequence_step"]) == (2, 1) and 0 < dev["lc_sequence_short"] <= dev["lc_candidates"]
    assert dev["lc_accepted"] == host["lc_accepted"] > 0
    # W = 0 is the run without the flag, key for key (the clocks aside)
    plain = loop.run(lc_gate="appearance", **KW)
    zero = loop.run(lc_gate="appearance", lc_sequence=0, **KW)
    assert set(plain) == set(zero) and "lc_sequence" not in zero
    for key in plain:  # (every count, name and flag; the clocks are floats)
        if isinstance(plain[key], (int, str, bool, type(None))):
            assert plain[key] == zero[key], key
    assert plain["lc_pairs"] == zero["lc_pairs"] and zero["err_lc_m"] == pytest.approx(plain["err_lc_m"], rel=1e-6)
    for bad in (dict(lc_gate="geometric", lc_sequence=2), dict(lc_gate="appearance", lc_sequence=9),
                dict(lc_gate="appearance", lc_sequence=2, lc_sequence_step=6)):
        with pytest.raises(ValueError):
            loop.run(**dict(KW, **bad))
