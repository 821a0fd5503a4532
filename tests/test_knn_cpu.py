"""k-nearest-neighbour up-sampling without a GPU: the host restatement (pasco_amd/grad/host.py knn_*) against the independent
references of tests/knn_cases.py, the drop-in `knn_up` / `kNN` / `index_points` of pasco_amd/grad/knn.py on CPU tensors, and the
MinkUNet-shaped network through the CPU checker backend.  The same checks run on the pk_* kernels in tests/test_hip_knn.py."""
import pytest
import torch

from pasco_amd.grad import knn as K
from tests import knn_cases as kc

CPU = torch.device("cpu")


@pytest.mark.parametrize("case", kc.sizes_cases(), ids=[c[0] for c in kc.sizes_cases()])
def test_search_sizes_against_the_all_pairs_loop(case):
    name, cand, q, k, grid = case
    kc.check_search(CPU, cand, q, k, grid, what=name)


@pytest.mark.parametrize("case", kc.edge_cases(), ids=[c[0] for c in kc.edge_cases()])
def test_search_edges_against_the_all_pairs_loop(case):
    name, cand, q, k, grid = case
    kc.check_search(CPU, cand, q, k, grid, what=name)


def test_search_edge_expectations():
    kc.check_edge_expectations(CPU)


@pytest.mark.parametrize("k", kc.KS)
def test_weights_against_fp64(k):
    kc.check_weights(CPU, k)


def test_forward_and_backward_against_fp64():
    for c in (1, 4, 33):
        kc.check_forward(CPU, c)
        kc.check_backward(CPU, c)
    kc.check_forward(CPU, 5, k=1)
    kc.check_forward(CPU, 5, k=16)
    kc.check_backward(CPU, 5, k=16)


@pytest.mark.parametrize("k", kc.KS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_knn_up_against_the_fp64_restatement(k, dtype):
    kc.check_knn_up(CPU, k, dtype)


def test_gradcheck_in_fp64():
    vox, q = kc.recipe()
    v, p = torch.from_numpy(vox).double(), torch.from_numpy(q[:40]).double()
    f = torch.randn(vox.shape[0], 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1), requires_grad=True)
    for k in (1, 3):
        assert torch.autograd.gradcheck(lambda t: K.knn_up(k)(v, t, p), (f,))


def test_grad_modes_give_the_same_bits():
    kc.check_grad_modes(CPU)


def test_refusals():
    kc.check_refusals(CPU)


def test_unet_gradients_against_the_dense_fp64_twin(oracle_registered):
    """Through the CPU checker backend (fp32 convolutions): the transposed convolution onto the encoder's map, the concatenation
    on one map and the two up-samplings, at the bound the GPU test holds."""
    kc.check_net(CPU)
