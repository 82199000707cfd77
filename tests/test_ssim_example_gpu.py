"""examples/fit_texture_photometric.py runs end to end on the GPU at a small size and lowers its loss."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

pytestmark = pytest.mark.gpu


def test_fit_texture_photometric_example(device, tmp_path):
    import fit_texture_photometric
    result = fit_texture_photometric.fit(steps=25, size=48, device=str(device), out=str(tmp_path))
    assert result["final_loss"] < result["initial_loss"]
    assert result["final_texel_error"] < result["initial_texel_error"]
    assert os.path.exists(os.path.join(str(tmp_path), "fitted.png"))
