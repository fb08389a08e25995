"""CPU checks of the one-stage heads' inference (no GPU), against the REFERENCE's own outputs
(tests/golden/dense_predict.npz, made by gen_dense_golden.py): the heads' torch candidates
(FCOSHead.image_candidates, AnchorHead.image_candidates on CPU tensors) followed by the oracle's
numpy multiclass NMS equal the reference's predict_single_image -- labels exact and in order,
scores rtol 1e-6, boxes rtol 2e-6 / atol 1e-4 (the bars of tests/test_gpu_whole_fcos.py).  The
multiclass NMS of the package runs on the HIP device only, and AnchorHead's decode is a HIP op:
here the oracle's numpy param2bbox and anchor grid stand in for them.  This pins image_candidates,
the oracle of tests/test_gpu_dense.py, to the reference, and the per-level tables of
dense_inputs to image_candidates."""
import numpy as np
import pytest
import torch

import dense_inputs as di
import oracle

TAGS = list(di.PREDICT_CASES)


def build_head(tag):
    c = di.PREDICT_CASES[tag]
    if c['kind'] == 'retina':
        from frcnn_amd.heads.retina_head import RetinaHead
        args, kw = di.retina_head_args(c)
        return RetinaHead(*args, **kw)
    from frcnn_amd.heads.fcos_head import FCOSHead
    return FCOSHead(**di.fcos_head_kwargs(c))


def cpu_candidates(head, tag, b, monkeypatch):
    """(boxes [n, 4], scores [n, C], factor [n] or None, per-level tables) of image b through the
    head's own image_candidates on CPU tensors."""
    from frcnn_amd import utils
    from frcnn_amd.config import ConfigDict
    c = di.PREDICT_CASES[tag]
    cls, reg, ctr = di.predict_inputs(tag)
    lc, lr = [torch.from_numpy(x[b]) for x in cls], [torch.from_numpy(x[b]) for x in reg]
    meta, cfg = di.METAS[b], ConfigDict(c['test_cfg'])
    if c['kind'] == 'retina':
        monkeypatch.setattr(utils, 'param2bbox', di.cpu_param2bbox)
        anchors = di.cpu_anchors(head)
        sc, bx, valid = head.image_candidates(lc, lr, anchors, meta, cfg)
        levels = di.retina_levels(head, lc, lr, anchors, meta, c['test_cfg'], di.cpu_param2bbox)
        sel_sc = torch.cat([lv['score'][:, lv['sel']] for lv in levels], 1)
        sel_bx = torch.cat([lv['box'][:, lv['sel']] for lv in levels], 1)
        sel_v = torch.cat([lv['valid'][lv['sel']] for lv in levels])
        assert torch.equal(sel_sc, sc) and torch.equal(sel_bx, bx)
        assert valid is None or torch.equal(sel_v, valid)
        keep = valid if valid is not None else torch.ones(sc.shape[1], dtype=torch.bool)
        return bx[:, keep].t().numpy(), sc[:, keep].t().numpy(), None, levels
    lt = [torch.from_numpy(x[b]) if x is not None else None for x in ctr]
    bx, sc, ct = head.image_candidates(lc, lr, lt, meta, cfg)
    levels = di.fcos_levels(head, lc, lr, lt, meta, c['test_cfg'])
    assert torch.equal(torch.cat([lv['score'][:, lv['sel']] for lv in levels], 1), sc)
    assert torch.equal(torch.cat([lv['box'][:, lv['sel']] for lv in levels], 1), bx)
    if ct is not None:
        assert torch.equal(torch.cat([lv['ctr'][lv['sel']] for lv in levels]), ct)
    return bx.t().numpy(), sc.t().numpy(), ct.numpy() if ct is not None else None, levels


def test_cases_cover_the_issue():
    kinds = [c['kind'] for c in di.PREDICT_CASES.values()]
    assert {'fcos', 'gfl', 'retina'} == set(kinds)
    assert {c['test_cfg']['nms_type'] for c in di.PREDICT_CASES.values()} == {'strict', 'official'}
    assert any(c['test_cfg']['min_bbox_size'] > 0 for c in di.PREDICT_CASES.values())
    assert di.METAS[0]['img_shape'] != di.METAS[1]['img_shape']
    assert di.METAS[0]['scale_factor'] != di.METAS[1]['scale_factor']
    assert di.PREDICT_CASES['retina']['A'] == 9 and di.PREDICT_CASES['gfl']['head']['loss_dfl']['cls_channels'] == 16
    assert 'loss_centerness' in di.PREDICT_CASES['fcos_ctr']['head']
    assert 'loss_centerness' not in di.PREDICT_CASES['fcos_noctr']['head']


@pytest.mark.parametrize('b', [0, 1])
@pytest.mark.parametrize('tag', TAGS)
def test_torch_path_vs_reference(golden, monkeypatch, tag, b):
    z = golden('dense_predict.npz')
    c = di.PREDICT_CASES[tag]
    head = build_head(tag)
    boxes, scores, factor, levels = cpu_candidates(head, tag, b, monkeypatch)
    assert di.check_gaps(levels, c['test_cfg']['pre_nms']) > di.GAP
    assert any(0 < c['test_cfg']['pre_nms'] < int(lv['cand'].sum()) for lv in levels)  # a level is cut
    if tag == 'fcos_ctr':
        assert any(not bool(lv['cand'].all()) for lv in levels)  # the min-size filter drops columns
    cfg = c['test_cfg']
    kb, ks, kl = oracle.multiclass_nms(boxes, scores, list(range(c['C'])), cfg['nms_iou'], cfg['min_score'],
                                       cfg['max_per_img'], factor, mode=cfg['nms_type'])
    rb, rs, rl = (z['{}_{}_{}'.format(tag, k, b)] for k in ('boxes', 'scores', 'labels'))
    assert len(rs) > 3
    np.testing.assert_array_equal(kl + 1, rl)
    np.testing.assert_allclose(ks, rs, rtol=1e-6, atol=0)
    np.testing.assert_allclose(kb, rb, rtol=2e-6, atol=1e-4)
