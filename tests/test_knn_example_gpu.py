"""examples/estimate_scan_normals.py on the MI355X: the normals of the ellipsoid cloud from knn_points' neighbours.

At 2000 points and K = 16 the same script gives a mean angle of 2.232189 degrees to the analytic normals on the host
torch path in float64 (measured there; the mean includes the one sample in a hundred that the sphere mesh's pole-fan
quirk puts inside the ellipsoid).  The device may exceed it by 10 %: float32 swaps neighbours at near-ties, which
exchanges points that are almost equally distant."""
import pytest

import knn_reference as kref

pytestmark = pytest.mark.gpu
HOST_FLOAT64_MEAN_DEGREES = 2.232189


def test_scan_normals_example(tmp_path):
    example = kref.load_example()
    out = tmp_path / "normals.xyz"
    mean, worst, cloud, normals = example.estimate(points=2000, neighbours=16, device="cuda:0", out=str(out))
    print("mean %.6f deg (host float64: %.6f), max %.3f deg" % (mean, HOST_FLOAT64_MEAN_DEGREES, worst))
    assert cloud.is_cuda and normals.shape == (2000, 3)
    assert mean <= 1.1 * HOST_FLOAT64_MEAN_DEGREES
    rows = out.read_text().splitlines()
    assert len(rows) == 2000 and all(len(row.split()) == 6 for row in rows)
    first = [float(v) for v in rows[0].split()]
    assert abs(sum(v * v for v in first[3:]) - 1.0) <= 1e-4
    angles, on_surface = example.angles_to_analytic(cloud, normals)
    assert int(on_surface.sum()) >= 1950 and float(angles[on_surface].mean()) < mean
