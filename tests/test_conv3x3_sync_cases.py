"""The integer cases of tests/test_gpu_conv3x3_sync.py, checked without a GPU: the module imports,
and its inputs keep every Winograd intermediate and every partial sum exactly representable in
f32, so that `torch.equal` against the float64 convolution is the right demand."""
import torch

import test_gpu_conv3x3_sync as sync


def _all_cins():
    return [s[1] for s in sync.ALTERNATING_SHAPES + sync.PROLOGUE_SHAPES] + [sync.LEVELS_CIN]


def test_sums_stay_below_2_to_24():
    # |x| <= 3, |w| <= 8, 9 taps, cin channels, |bias| <= 5: any order of summation is exact.  The
    # Winograd side: |V| <= 4 |x| = 12 and |U| <= 9/4 |w| = 18 per element, 16 cin products of at
    # most 216 per position and output, and the output transform adds at most 9 positions.
    for cin in _all_cins():
        assert sync.cases_bound(cin) < 2 ** 24
        assert 9 * cin * 12 * 18 + sync.BIAS_MAX < 2 ** 24


def test_weights_are_quarter_safe_and_inputs_integers():
    # U = G g G^T halves twice: w = 4 x integer keeps U an integer
    g = torch.Generator().manual_seed(1)
    xs, wt, bias = sync._draw(g, 1, 8, 64, [(3, 5)])
    assert torch.equal(wt, (wt / 4).round() * 4) and float(wt.abs().max()) <= sync.W_MAX
    assert torch.equal(xs[0], xs[0].round()) and float(xs[0].abs().max()) <= sync.X_MAX
    assert torch.equal(bias, bias.round()) and float(bias.abs().max()) <= sync.BIAS_MAX


def test_small_references_are_integers():
    for shape in sync.PROLOGUE_SHAPES:
        n, cin, cout, h, w = shape
        g = torch.Generator().manual_seed(7500 + cin)
        (x,), wt, b = sync._draw(g, n, cin, cout, [(h, w)])
        want = sync._exact(x, wt, b, False)
        assert torch.equal(want, want.round()) and float(want.abs().max()) <= sync.cases_bound(cin)
    for c in sync._levels_case():
        assert c['xs'][-1].shape[2:] == (3, 4)
        for want in c['want']:
            assert torch.equal(want, want.round()) and float(want.abs().max()) <= sync.cases_bound(sync.LEVELS_CIN)
