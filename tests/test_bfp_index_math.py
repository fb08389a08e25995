"""CPU check of the BFP kernels' index arithmetic (csrc/bfp.hip pool_start / pool_end /
nearest_of and the backward's win_first / win_last), restated in frcnn_amd.necks, against
what torch's own adaptive max pool and nearest interpolation do, for every (in, out) size
pair up to 96: an arange row probes the windows (the max of an increasing row is its
window's last cell, of a decreasing row its first) and the nearest rule's source cells."""
import numpy as np
import torch
import torch.nn.functional as F

from frcnn_amd.necks import adaptive_window, adaptive_windows_of, nearest_source

N = 96


def test_adaptive_windows_match_torch():
    for n_in in range(1, N + 1):
        row = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
        for n_out in range(1, N + 1):
            last = F.adaptive_max_pool2d(row, (1, n_out)).view(-1).numpy().astype(np.int64)
            # the decreasing row holds n_in - 1 - p at cell p: a window's maximum is at its first cell
            first = (n_in - 1 - F.adaptive_max_pool2d(row.flip(3), (1, n_out)).view(-1).numpy()).astype(np.int64)
            win = [adaptive_window(o, n_in, n_out) for o in range(n_out)]
            assert [e - 1 for _, e in win] == last.tolist(), (n_in, n_out)
            assert [s for s, _ in win] == first.tolist(), (n_in, n_out)


def test_adaptive_windows_along_height_too():
    row = torch.arange(13, dtype=torch.float32).view(1, 1, 13, 1)
    got = F.adaptive_max_pool2d(row, (4, 1)).view(-1).tolist()
    assert got == [adaptive_window(o, 13, 4)[1] - 1 for o in range(4)]


def test_windows_containing_a_cell_are_the_inverse():
    for n_in in range(1, N + 1):
        for n_out in range(1, N + 1):
            win = [adaptive_window(o, n_in, n_out) for o in range(n_out)]
            for p in range(n_in):
                want = [o for o, (s, e) in enumerate(win) if s <= p < e]
                first, last = adaptive_windows_of(p, n_in, n_out)
                assert want == list(range(first, last + 1)), (n_in, n_out, p)


def test_nearest_source_matches_torch():
    for n_in in range(1, N + 1):
        row = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
        for n_out in range(1, N + 1):
            got = F.interpolate(row, size=(1, n_out), mode='nearest').view(-1).numpy().astype(np.int64)
            assert [nearest_source(d, n_in, n_out) for d in range(n_out)] == got.tolist(), (n_in, n_out)


def test_nearest_source_is_monotone():
    """The backward gathers a source cell's destinations as one contiguous range."""
    for n_in in range(1, N + 1):
        for n_out in range(1, N + 1):
            src = [nearest_source(d, n_in, n_out) for d in range(n_out)]
            assert all(a <= b for a, b in zip(src, src[1:])), (n_in, n_out)
