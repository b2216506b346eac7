"""`oard_wgrad_scratch_bytes` never decreases with the row count (host arithmetic, no device).

The training scratch is sized once per topology from N, E + 1 and A + 1 rows (`make_train_ws`, csrc/oard_train_stages.h) and then serves
weight-gradient products of E, A and per-object row counts, each of which checks its own need.  The exact need is not monotone in the
rows (a chunk's rows are rounded up, the plan changes kernels at 16384 rows), so a ragged batch whose row count sat just below a drop -
704 x 208 columns needed more for 10880 rows than for 10881 - failed its step with "workspace too small", as a dataset-fed run did.  The size is
now an upper bound that is monotone, which makes "sized for more rows" imply "fits"."""
import numpy as np

from oareactdiff_amd import _capi
from oareactdiff_amd.build import build

#: (dY columns, X columns) of the sweep's products at the production widths (HP 208, WP 704, RP 96) and the test widths
SHAPES = [(704, 208), (208, 208), (208, 704), (624, 96), (208, 96), (624, 208), (416, 208), (208, 16), (16, 208), (32, 16), (48, 112)]


def test_scratch_bytes_is_monotone_in_rows():
    build()
    f = _capi.lib().oard_wgrad_scratch_bytes
    rows = list(range(1, 40000, 1)) + list(range(40000, 2_000_000, 4093))
    for y, x in SHAPES:
        need = np.array([f(y, x, r) for r in rows], dtype=np.int64)
        drops = np.nonzero(np.diff(need) < 0)[0]
        assert drops.size == 0, f"{y} x {x}: {rows[drops[0]]} rows need {need[drops[0]]} bytes, {rows[drops[0] + 1]} rows {need[drops[0] + 1]}"
        assert need[0] >= 4 * 1024 * 1024                  # the small-output path's floor


def test_the_shape_that_failed():
    build()
    f = _capi.lib().oard_wgrad_scratch_bytes
    assert f(704, 208, 10881) >= f(704, 208, 10880) and f(208, 208, 16385) >= f(208, 208, 16384) >= f(208, 208, 16383)
