"""bench.py's command line off the GPU: --dump-outputs writes the step's returned arrays as
float32 .npy files, and the options that belong to --full refuse a plain run."""
import os
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_loss_dict_and_sum(tmp_path):
    import bench
    losses = {'loss_a': torch.tensor(1.5, dtype=torch.float64, requires_grad=True), 'loss_c': torch.tensor(3.0)}
    out = tmp_path / 'nested' / 'dir'
    bench.dump_outputs(str(out), {'losses': losses})
    assert sorted(os.listdir(out)) == ['loss.npy', 'loss_a.npy', 'loss_c.npy']
    for name, want in (('loss_a', 1.5), ('loss_c', 3.0), ('loss', 4.5)):
        a = np.load(out / (name + '.npy'))
        assert a.dtype == np.float32 and a.shape == () and a == want
    # train mode: the step's loss
    bench.dump_outputs(str(tmp_path / 't'), {'loss': torch.tensor(7.0)})
    assert os.listdir(tmp_path / 't') == ['loss.npy'] and np.load(tmp_path / 't' / 'loss.npy') == 7.0


def test_dump_rois_needs_full():
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--dump-rois', 'unused.npz'],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and 'needs --full' in r.stderr
