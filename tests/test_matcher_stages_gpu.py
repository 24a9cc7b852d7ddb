"""The matcher's kernels stage by stage against a float64 reference (tests/stagewise.py).

A cached forward runs one stage at a time on one workspace (onepose_match_cached_stages); after
each GNN layer the token states are read where onepose_match_workspace_region says they are, then
the final descriptors, the score matrix S and conf_matrix.  Every one of them must lie within
K = 4 times the float32 numpy oracle's own error against the float64 run of the same oracle
(floored at 2 float32 ulps), so a subtly wrong partial sum, InstanceNorm statistic or softmax
statistic fails at the layer it happens in -- under raw weights, where the attention path is not
damped 30x on its way to the outputs (tests/test_stagewise_host.py shows both halves of that).
The existing end-to-end contract (tests/parity.py) is asserted on the same run.

Cases (stagewise.CASES), the smallest shapes reaching each code path:
  65x97 raw / well-conditioned   tile edges at 33 / 65 / 97 rows; the well-conditioned one has
                                 real matches, so a stage and an index failure show together
  1x7 L=2                        single-token side: InstanceNorm variance 0
  300x1000                       partial last KV chunk, the 32-row fp32 QKV tile
  200x330 L=6 B=6                B > 4: kv_reduce + m_fold, one object for the batch, the batch
                                 stride of the state layout
  900x2756                       44 64-row tiles of the 3D side: the 128-row stand-in QKV tile,
                                 its last tile's second sub-tile holding 4 rows of either side
  1000x2692                      43 tiles: that sub-tile empty, 40 rows of the 2D side in the last
  128x256 L=12                   gat_kernel<16>
The bf16 mode is out of scope: it is not fp32-accurate by design."""
import numpy as np
import pytest

import stagewise as SW
from parity import ATOL, assert_pred_equal

pytestmark = pytest.mark.gpu

GPU_CASES = ["65x97-raw", "65x97-wc", "1x7-raw", "300x1000-raw", "200x330-b6-raw", "900x2756-raw",
             "1000x2692-raw", "128x256-l12-raw"]
PRECISIONS = {"fp32": 0, "fp32_split": 2}   # the split mode claims fp32 accuracy: the same K


def check(case, precision, device, flags=0):
    ref64, ref32 = SW.reference(case)
    got = SW.gpu_stages(case, PRECISIONS[precision], device, flags)
    title = f"{case} {precision}" + (" gat-tables" if flags else "")
    SW.assert_stages(title, got, ref64, ref32)
    # the end-to-end contract on the same run, against the float32 oracle as everywhere else
    for b, (g, r) in enumerate(zip(got["pred"], ref32["pred"])):
        assert_pred_equal(g, r, f"{title} frame {b}")
    np.testing.assert_allclose(got["conf"], ref32["conf"], rtol=0, atol=ATOL)
    if case.endswith("-wc"):
        assert (got["pred"][0]["matches0"] > -1).sum() >= 20


@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("case", GPU_CASES)
def test_stages_vs_float64(case, precision, device):
    check(case, precision, device)


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_stages_vs_float64_gat_tables(precision, device):
    """ONEPOSE_OBJ_GAT_TABLES: GAT layers 1-3 from the object's prefix tables "differ in rounding
    only" from reading the leaves (include/onepose_hip.h), so they get the same K."""
    from onepose_amd import _lib
    check("65x97-raw", precision, device, flags=_lib.OBJ_GAT_TABLES)


def test_stagewise_forward_is_the_one_call_forward(device):
    """The stage-at-a-time run the tests above read from gives the bits of the one-call cached
    forward (so what they check is what the product computes), and the region query refuses the
    final descriptors before ONEPOSE_STAGE_FINAL."""
    import torch

    from onepose_amd import _lib, matcher, synthetic
    case = "65x97-wc"
    got = SW.gpu_stages(case, 0, device)
    sd, data = SW.case_inputs(case)
    m = matcher.from_state_dict(sd, dict(synthetic.DEFAULT_HPARAMS)).to(device)
    with torch.no_grad():
        pred, conf = m({k: torch.from_numpy(v).to(device) for k, v in data.items()})
    np.testing.assert_array_equal(conf.cpu().numpy(), got["conf"])
    for k, v in pred.items():
        np.testing.assert_array_equal(v.cpu().numpy(), got["pred"][0][k], err_msg=k)
    lib = _lib.load()
    with pytest.raises(_lib.OnePoseError):
        _lib.workspace_region(lib, 1, 65, 97, 8, True, 0, _lib.REGION_DESC2D,
                              _lib.STAGE_LAYER0 + 11)
