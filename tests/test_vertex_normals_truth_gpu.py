"""The vertex-normal kernels (csrc/mesh_ops.hip: k_vertex_normals, k_vertex_normals_backward) against a float64 truth.

tests/vertex_normals_reference.py holds the restatement (the scatter formulation), the meshes and the bound;
tests/test_vertex_normals_truth_host.py checks without a GPU that no vertex sum sits near the normalisation's eps.
Every case is two images with random upstream weights, forward and backward through compute_vertex_normals, and per
tensor (the normals, d vertices) and image

    |kernel - f64|[b]  <=  K * r * max|f64[b]|  +  1e-7 * max|f64|          (K = 8)

r being the float32 restatement's worst per-image relative error on the same mesh and weights.

Cases: open fans whose hub has exactly 7, 8, 9, 16, 17 and 40 incident corners (one trip of the eight lanes, exactly one,
one entry into the second, two full trips, one entry into the third, five); random meshes of V = 1, 31, 32, 33 and 257
vertices (2 V groups of eight lanes, 32 groups to a 256-thread block: half a block, a block edge between the two
images, a full pair of blocks, a group across the edge, seventeen blocks with the last partly empty); a triangle
(i, i, j); a zero-area triangle of three distinct ids on its own (sums exactly zero: the dn / eps branch, gradients of
~1e6, judged on their own) next to isolated vertices (normal and gradient exactly 0); triangles with an id out of
range (judged against the truth, and bit for bit against the mesh without them); the 5k-vertex sphere.

MEASURED on the MI355X (ratio = kernel's worst per-image relative error / r; r is 6e-8 .. 7e-7 on these meshes):

    case      normals  d vertices      case          normals  d vertices      case                 normals  d vertices
    fan-7     1.00     2.34            size-31       0.92     1.43            repeated-id          1.17     1.01
    fan-8     1.22     1.00            size-32       0.60     0.81            zero-area / fan      1.07     0.69
    fan-9     1.00     1.52            size-33       1.02     0.75            zero-area / eps      exact 0  1.00
    fan-16    1.55     1.26            size-257      0.84     1.00            out-of-range         1.08     1.00
    fan-17    0.99     0.96            size-1        exact 0  exact 0         sphere (5k)          1.23     1.11
    fan-40    1.29     1.82

The worst is 2.34.  Swapping k1 / k2 in the j = k2 term of k_vertex_normals_backward (not committed) fails every mesh but
V = 1 at 2.5e5 .. 1.4e6 times the allowance.
"""
import pytest
import torch

import vertex_normals_reference as vr
from pytorch_mesh_renderer_amd.common import meshes

pytestmark = pytest.mark.gpu


def kernel_run(c, device, triangles=None):
    v = c.vertices.clone().to(device).requires_grad_(True)
    n = meshes.compute_vertex_normals(v, (c.triangles if triangles is None else triangles).to(device))
    (n * c.weights.to(device)).sum().backward()
    return {"normals": n.detach(), "d_vertices": v.grad}


@pytest.mark.parametrize("name", vr.NAMES)
def test_vertex_normals_against_the_float64_truth(device, name):
    c = vr.case(name)
    got = kernel_run(c, device)
    for k, t in got.items():
        assert t.shape == c.vertices.shape and t.dtype == torch.float32 and bool(torch.isfinite(t).all()), k
    over, _ = c.compare(got)
    assert not over, "\n".join(over)
    again = kernel_run(c, device)      # no atomics: the same bits every time
    assert torch.equal(again["normals"], got["normals"]) and torch.equal(again["d_vertices"], got["d_vertices"])


def test_isolated_and_zero_sum_vertices_are_exactly_zero(device):
    c = vr.case("zero-area")
    got = kernel_run(c, device)
    z, iso = c.groups["zero-area"], c.groups["isolated"]
    assert not bool(got["normals"][:, z + iso].any())
    assert not bool(got["d_vertices"][:, iso].any())
    assert float(got["d_vertices"][:, z].abs().max()) > 1e5
    c = vr.case("size-1")              # one vertex, the triangle (0, 0, 0)
    got = kernel_run(c, device)
    assert not bool(got["normals"].any()) and not bool(got["d_vertices"].any())


def test_out_of_range_triangles_are_as_good_as_absent(device):
    """Bit for bit the mesh without them.  The skipped triangles stand at the END of the list here: an entry's place in
    its vertex's adjacency row decides which of the eight lanes adds it, so taking a triangle out of the middle
    re-associates the sums of its in-range vertices (the case of the module's parametrised test has one in the middle
    and is held to the truth instead)."""
    c = vr.case("fan-17")
    V = c.vertices.shape[1]
    bad = torch.tensor([[0, 4, V + 3], [-1, 0, 2], [V, V + 1, V + 2], [5, 2 ** 31 - 1, 6]], dtype=torch.int32)
    want = kernel_run(c, device)
    got = kernel_run(c, device, torch.cat([c.triangles, bad]))
    assert torch.equal(got["normals"], want["normals"]) and torch.equal(got["d_vertices"], want["d_vertices"])
