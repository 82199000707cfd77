"""Fuzz of mr_rasterize_backward on random triangle soups (GPU; not collected by pytest): the lane-accumulating kernel
with its pipelined row loop and the deterministic mode's run kernel, EACH against the float64 truth
(oracle/truth64.py) within the scene's own bound K_scene (2^-24 noise + 1e-7) -- backward_fuzz.raster_trial; K_scene
is calibrated by the oracle on the same G-buffer, never by a kernel (tests/raster_backward_scenes.py).  A fixed-seed
slice runs inside `pytest -m gpu` (tests/test_backward_truth_gpu.py).

    python tests/fuzz_raster_backward_gpu.py [seed]

120 soups of backward_fuzz.soup's full-size recipe (slivers, one-pixel triangles, repeated and degenerate triangles,
images up to 420x300, 1..3 images per call); the G-buffer is the device's own (bit-identical to the oracle's,
tests/fuzz_raster_gpu.py)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import backward_fuzz

TRIALS = 120
seed = int(sys.argv[1]) if len(sys.argv) > 1 else 5
t0 = time.time()
report = backward_fuzz.run(backward_fuzz.raster_trial, TRIALS, seed, progress=20)
for line in report.failures[:40]:
    print("MISMATCH", line)
bad = bool(report.failures) or report.with_gradients < TRIALS // 2 or report.det_skipped > TRIALS // 4
print("FUZZ", "FAILED" if bad else "OK", "%d soups (%d with gradients, %d without the deterministic run), %d values beyond the bound, "
      "%.0f s; worst error / bound per kernel: %s" % (TRIALS, report.with_gradients, report.det_skipped, len(report.failures),
                                                     time.time() - t0, report.summary()))
sys.exit(1 if bad else 0)
