"""Pin the CPU oracle's training coarse query (orc.query_coarse_static) and torch autograd through it to golden G18: numbers captured
from the reference's own run_network_NeRFW(..., typ='coarse', test_time=False) by tests/golden/make_golden_coarse_static.py.  The
bound is the one tests/test_oracle_golden.py holds the network goldens to (rtol = atol = 1e-6)."""
import torch

from dfnet_amd import synthetic as syn
from tests.test_oracle_golden import close, tt
from oracle import nerfh_oracle as orc

T = torch.from_numpy


def test_g18_coarse_static_query_and_its_autograd(gold):
    g = gold("g18_coarse_static")
    c = tt(syn.nerfh_weights(0)[0])
    assert g["raw4"].shape == (3, 5, 4) and g["g_pts"].shape == (3, 5, 3) and g["g_viewdirs"].shape == (3, 3)
    p, v = T(g["pts"]).clone().requires_grad_(True), T(g["viewdirs"]).clone().requires_grad_(True)
    out = orc.query_coarse_static(c, p, v)
    close(out, g["raw4"])
    (out * T(g["G"])).sum().backward()
    close(p.grad, g["g_pts"])
    close(v.grad, g["g_viewdirs"])
