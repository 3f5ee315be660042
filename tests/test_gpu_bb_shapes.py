"""pl_features_sweep, pl_features_sweep_u16 and pl_features_level on the MI355X against the oracle, on the shape zoo of
tests/golden/bb_shapes.npz: regions on the hull paths' switch (31 / 32 / 33 rows) and far beyond it, shapes rejected by exactly
one predicate, twins on the two sides of each bound, holes open and closed, clear_border at zero and one pixel, the candidate /
crop / output table limits and their status words, the sweep's control flow (max_number, min_separation 0, same-level
duplicates, discs completed at different levels), window geometry, and the uint16 source.  The checks are
tests/bb_shape_checks.py; the emulator runs a subset of them in tests/test_emulated_bb_shapes.py."""
from __future__ import annotations

import numpy as np
import pytest

import bb_shape_checks as checks

pytestmark = pytest.mark.gpu

WINDOWS = ["rows31_32_33", "tall35", "tall64", "tall67", "one_predicate_each", "edges.area_hi", "edges.area_lo",
           "edges.symmetric", "edges.solid", "holes", "border.touch", "border.near", "levels", "dedup", "many.blobs40",
           "many.discs10", "geometry.97x150", "geometry.150x97", "geometry.160x160", "geometry.161x130", "geometry.words"]


def test_every_window_of_the_golden_is_run(golden):
    assert checks.names(golden("bb_shapes")) == WINDOWS


@pytest.mark.parametrize("name", WINDOWS)
def test_bb_finder_on_shape_window(golden, dev, name):
    checks.check_window(dev, golden("bb_shapes"), name)


@pytest.mark.parametrize("ks", [(0, 1), (2,)], ids=["400x400", "150x400_clipped"])
def test_bb_centroids_on_uint16_frames(golden, dev, ks):
    checks.check_u16(dev, golden("bb_shapes"), ks)
