"""Pin the oracle's three restatements of raw2outputs_NeRFW (coarse_weights, composite_coarse_train, composite_fine) to the reference's
own outputs AND to the reference's own autograd with respect to raw and z_vals (tests/golden/g17_raw2outputs.npz, written by
tests/golden/make_golden_raw2outputs.py): the GPU tests of dfn_raw2outputs / dfn_raw2outputs_backward take these functions as truth.

Values: the bound tests/test_oracle_golden.py applies to G4 (rtol = atol = 1e-6).  Gradients: 1e-5 relative maximum."""
import numpy as np
import pytest
import torch

from tests import raw2outputs_cases as rc

T = torch.from_numpy
G17_MODES = {"m1": "raw1", "m2": "raw4", "m2w": "raw4", "m3": "raw9", "m3w": "raw9", "m3t": "raw9"}


def relmax(a, b):
    a, b = a.detach().double(), torch.as_tensor(b).double()
    assert a.shape == b.shape
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("tag", sorted(G17_MODES))
def test_g17_oracle_reproduces_the_reference(gold, tag):
    g = gold("g17_raw2outputs")
    raw, z = T(g[G17_MODES[tag]]), T(g["z"])
    assert z.shape == (6, 12) and bool((z[:, 1:] >= z[:, :-1]).all())
    if tag in ("m1", "m2"):
        sig = raw[..., -1]
        assert bool((sig < 0).any()) and bool((sig > 0).any())    # the relu matters
    ch = rc.MODES[tag][0]
    out = rc.oracle(tag, raw, z)
    # what the reference returns and what it returns None for
    present = {k[len(tag) + 1:] for k in g if k.startswith(tag + "_")} - {"graw", "gz"}
    assert present == set(rc.OUTPUTS[ch]) | ({"tsig"} if ch == 9 else set()) | ({"beta"} if ch == 4 else set())
    for k in rc.OUTPUTS[ch]:
        np.testing.assert_allclose(out[k].numpy(), g[f"{tag}_{k}"], rtol=1e-6, atol=1e-6, err_msg=k)
    if ch == 4:
        assert not g[f"{tag}_beta"].any() and g[f"{tag}_beta"].shape == (6,)      # "just to fake a return"
    if ch == 9:
        assert np.array_equal(g[f"{tag}_tsig"], raw[..., 7].numpy())
    # the gradient of sum_k (output_k * G_k) over every output the mode returns (transient_sigmas = raw[..., 7] among them)
    G = {k: T(g["G_" + k]) for k in rc.OUTPUTS[ch]}
    graw, gz = rc.oracle_grads(tag, raw, z, G)
    if ch == 9:
        graw = graw.clone()
        graw[..., 7] += T(g["G_tsig"])
    e_raw, e_z = relmax(graw, g[f"{tag}_graw"]), relmax(gz, g[f"{tag}_gz"])
    print(f"{tag}: oracle autograd vs the reference's: d raw {e_raw:.2e}, d z {e_z:.2e}")
    assert e_raw <= 1e-5 and e_z <= 1e-5
