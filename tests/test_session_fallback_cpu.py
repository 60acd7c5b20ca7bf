"""The recovery by feature matching inside the session (vh_session_set_fallback): what can be checked without a GPU -- every default is off, and the new
entry points are declared with a signature."""
import inspect


def test_fallback_is_off_by_default_everywhere():
    from velocity_amd import driver

    for fn in (driver.TrackerSession.__init__, driver.run_sequence, driver.run_sequences):
        par = inspect.signature(fn).parameters
        assert par["fallback"].default is False, fn
        assert par["fallback_params"].default is None, fn


def test_the_new_entry_points_are_declared_with_signatures():
    from velocity_amd import _lib

    for sym in ("vh_match_affine_batch", "vh_match_reserve_batch", "vh_session_set_fallback", "vh_session_recoveries"):
        assert sym in _lib.declared_symbols(), sym
        assert sym in _lib._SIGS, sym
    assert len(_lib._SIGS["vh_match_affine_batch"][1]) == 16
    assert len(_lib._SIGS["vh_match_reserve_batch"][1]) == 6


def test_the_driver_has_a_fallback_switch(monkeypatch):
    from velocity_amd import driver

    seen = {}
    monkeypatch.setattr(driver, "run_sequence", lambda *a, **k: seen.update(k))
    import numpy as np

    class Clip(dict):
        pass

    fr = np.zeros((2, 8, 8), np.uint8)
    monkeypatch.setattr(np, "load", lambda path: {"b_frames": fr, "b_q": 0, "b_K": 0, "b_times": 0})
    driver.main(["clip.npz"])
    assert seen["fallback"] is False
    driver.main(["clip.npz", "--fallback"])
    assert seen["fallback"] is True
