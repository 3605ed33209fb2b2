"""
Integrated variance reduction without a GPU: the closed form the engine uses (tests/ivr_oracle.py: closed) against its
definition (brute: M refits of the dense oracle with the candidate appended), and the library's export table.

Bar: 1e-12 absolute.  The identity is exact (the refit puts noise + jitter on the new point's diagonal, as the closed form's
denominator does); the gaps measured in float64 are <= 2.6e-15 for values of 0.36 - 0.57.  Every case also asserts that the
smallest latent variance is > 0, so that the oracle's clamp at 0 cannot hide a difference.
"""
import numpy as np
import pytest

import ivr_oracle as IO

CASES = [("RBF", 40, (6, 5), None), ("Matern52", 40, (6, 5), None), ("RationalQuadratic", 40, (6, 5), None),
         ("Matern52", 130, (13, 10), None), ("Matern52", 40, (6, 5), 7)]


@pytest.mark.parametrize("kind,N,shape,wseed", CASES)
def test_closed_form_is_the_definition(kind, N, shape, wseed):
    kp, _, _, X, _, G = IO.case(kind, N, shape)
    assert len(X) == N and np.array_equal(G[:3].numpy(), X[:3].numpy())
    w = None if wseed is None else IO.weights(G.shape[0], wseed)
    if w is not None:
        assert (w == 0.0).sum() >= 3 and w.max() <= 2.0 and w.min() >= 0.0
    vmin = IO.latent_var(kp, X, G).min()
    a_closed, a_brute = IO.closed(kp, X, G, w), IO.reference(kind, N, shape, "brute", wseed)
    gap = np.abs(a_closed - a_brute).max()
    print("%s N=%d grid %s weights %s: max a %.3f, min latent variance %.4f, max |closed - brute| %.2e"
          % (kind, N, shape, wseed, a_brute.max(), vmin, gap))
    assert vmin > 0.0
    assert gap <= 1e-12


def test_entry_is_exported():
    from gpim_amd import _lib
    assert "gpimhip_ivr_exact" in _lib.EXPORTS
    assert len(_lib._PROTOS["gpimhip_ivr_exact"][1]) == 13
