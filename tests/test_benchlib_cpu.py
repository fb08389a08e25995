"""tools/benchlib.py without a device: the repetition loop against a scripted timer, the rotation
and the window of the event-pair timer against a stubbed event pair, the dispatch rule, the row
fields, the limit, and that the tools which use it still import and have no timer of their own."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, 'tools')
_path = list(sys.path)
sys.path.insert(0, TOOLS)
import benchlib  # noqa: E402
sys.path[:] = _path  # collected with every run: the other tests (and the processes they spawn) keep their path

CONVERTED = ['bench_rpn_head1x1', 'bench_conv1x1', 'bench_conv3x3', 'bench_conv3x3_nchw', 'bench_conv3x3_variants',
             'bench_deform_conv', 'bench_roi_conv', 'bench_head_convs', 'bench_fcos', 'bench_gfl', 'bench_libra',
             'bench_dense_candidates', 'bench_select', 'bench_nms', 'bench_roi_align', 'bench_roi_bwd', 'bench_roi_sets',
             'bench_roi_order', 'probe_fpn_layout', 'probe_backbone_layout']
# bench_roi_align.py's cold and after-write arms interleave a cache-evicting pass with the launch
# inside one event pair and subtract an arm without the launch: no window of time_calls, so that
# event pair stays in the tool.  roi_dispatch_table.py times nothing itself: it hands a pool of
# recorded event pairs to ops.ROI_ALIGN_PROFILE, which records them around the launches of a step.
OWN_EVENT_PAIR = {'bench_roi_align.py', 'roi_dispatch_table.py'}


class ScriptedTimer:
    """Stands in for time_calls: hands out each side's scripted values and logs every call."""

    def __init__(self, sides, script, log):
        self.names = {id(v): k for k, v in sides.items()}
        self.script = {k: list(v) for k, v in script.items()}
        self.log, self.calls = log, []

    def __call__(self, fns, iters, sleep):
        name = self.names[id(fns)]
        self.calls.append((name, iters, sleep))
        self.log.append(('timed', name))
        return self.script[name].pop(0)


def scripted(script, per_side=2, log=None, **kw):
    log = [] if log is None else log
    sides = {k: [(lambda k=k, i=i: log.append(('call', k, i))) for i in range(per_side)] for k in script}
    timer = ScriptedTimer(sides, script, log)
    stat = benchlib.measure(sides, kw.pop('iters', 20), len(next(iter(script.values()))), timer=timer, **kw)
    return stat, timer, log


SCRIPT = {'parent': [5.0, 9.0, 7.0, 8.0, 6.0], 'fused': [4.0, 1.0, 3.0, 2.0, 10.0]}


def test_measure_returns_median_min_max_and_runs_per_side():
    stat, _, _ = scripted(SCRIPT, warmup=0)
    assert set(stat) == {'parent', 'fused'}
    assert tuple(stat['parent'][:3]) == (7.0, 5.0, 9.0) and stat['parent'].runs == SCRIPT['parent']
    assert tuple(stat['fused'][:3]) == (3.0, 1.0, 10.0) and stat['fused'].runs == SCRIPT['fused']
    assert (stat['fused'].median, stat['fused'].min, stat['fused'].max) == (3.0, 1.0, 10.0)


def test_measure_keeps_the_given_order_on_every_repetition():
    _, timer, _ = scripted(SCRIPT, warmup=0, iters=13, sleep=True)
    assert timer.calls == [('parent', 13, True), ('fused', 13, True)] * 5


def test_measure_reverses_the_odd_repetitions_when_asked():
    _, timer, _ = scripted(SCRIPT, warmup=0, reverse=True, sleep=False)
    assert [c[0] for c in timer.calls] == ['parent', 'fused', 'fused', 'parent', 'parent', 'fused', 'fused', 'parent',
                                           'parent', 'fused']
    assert {c[2] for c in timer.calls} == {False}


def test_measure_takes_the_calls_per_window_per_side():
    _, timer, _ = scripted(SCRIPT, warmup=0, iters={'parent': 3, 'fused': 60})
    assert timer.calls == [('parent', 3, True), ('fused', 60, True)] * 5


# ------------------------------------------------------------------------- the event-pair timer
def test_rotate_is_the_callable_itself_or_the_list_in_rotation():
    f, g, h = (lambda: 0), (lambda: 1), (lambda: 2)
    assert list(benchlib.rotate(f, 3)) == [f, f, f]
    assert list(benchlib.rotate([f, g, h], 7)) == [f, g, h, f, g, h, f]
    assert list(benchlib.rotate([f, g, h], 2)) == [f, g] and list(benchlib.rotate([f], 0)) == []


@pytest.fixture
def device_log(monkeypatch):
    """torch.cuda's event pair, hold and synchronise replaced by entries in a log; a pair reads 2 ms."""
    log = []

    class Event:
        def __init__(self, enable_timing):
            assert enable_timing

        def record(self):
            log.append('record')

        def elapsed_time(self, other):
            return 2.0
    monkeypatch.setattr(benchlib.torch.cuda, 'Event', Event)
    monkeypatch.setattr(benchlib.torch.cuda, 'synchronize', lambda: log.append('sync'))
    monkeypatch.setattr(benchlib.torch.cuda, '_sleep', lambda n: log.append(('sleep', n)))
    return log


def test_time_calls_rotates_inside_one_event_pair_behind_the_hold(device_log):
    fns = [(lambda i=i: device_log.append(i)) for i in range(3)]
    us = benchlib.time_calls(fns, 8, sleep=True)
    assert device_log == [('sleep', 100000000), 'record', 0, 1, 2, 0, 1, 2, 0, 1, 'record', 'sync']
    assert us == 2.0 * 1e3 / 8


def test_time_calls_warms_and_synchronises_before_the_window(device_log):
    us = benchlib.time_calls(lambda: device_log.append('f'), 4, sleep=False, warmup=3)
    assert device_log == ['f', 'f', 'f', 'sync', 'record', 'f', 'f', 'f', 'f', 'record', 'sync']
    assert us == 500.0


@pytest.mark.parametrize('warmup', [0, 1, 2, 3])
def test_measure_warms_every_callable_before_the_first_timed_call(device_log, warmup):
    _, _, log = scripted(SCRIPT, per_side=3, log=device_log, warmup=warmup)
    first = log.index(('timed', 'parent'))
    warm = log[:first]
    assert warm == [('call', side, i) for side in SCRIPT for i in range(3) for _ in range(warmup)] + ['sync'] * (warmup > 0)
    assert all(e[0] == 'timed' for e in log[first:])  # the scripted timer calls nothing


def test_compare_alternates_two_callables_without_the_hold(device_log):
    a, b = (lambda: device_log.append('a')), (lambda: device_log.append('b'))
    ma, mb, ra, rb = benchlib.compare(a, b, 4, 2, warmup=3, reps=2)
    window = lambda f, n: ['record'] + [f] * n + ['record', 'sync']  # noqa: E731
    assert device_log == ['a'] * 3 + ['b'] * 3 + ['sync'] + (window('a', 4) + window('b', 2)) * 2
    assert (ma, mb, ra, rb) == (500.0, 1000.0, [500.0, 500.0], [1000.0, 1000.0])


# ------------------------------------------------------------------------- the rule and the rows
def stats(**runs):
    return {k: benchlib.stat_of(v) for k, v in runs.items()}


def test_wins_needs_the_slowest_repetition_strictly_below_the_others_fastest():
    assert benchlib.wins(stats(a=[1, 2, 3], b=[3.5, 4, 5]), 'a', 'b') is True
    assert benchlib.wins(stats(a=[1, 2, 3], b=[3, 4, 5]), 'a', 'b') is False  # equality is not a win
    assert benchlib.wins(stats(a=[1, 2, 3], b=[3.5, 4, 5]), 'b', 'a') is False


def test_wins_is_false_for_overlapping_spreads_even_with_the_lower_median():
    s = stats(a=[1, 1, 1, 1, 6], b=[5, 7, 7, 7, 7])
    assert s['a'].median < s['b'].median
    assert benchlib.wins(s, 'a', 'b') is False and benchlib.wins(s, 'b', 'a') is False


def test_wins_docstring_names_the_exclusion_tables():
    for table in ('_CONV1X1_EXCLUDED', '_CONV1X1_PRE_EXCLUDED', '_CONV1X1_S2_EXCLUDED', '_CONV3X3_EXCLUDED',
                  '_CONV3X3_NCHW_EXCLUDED', '_HEAD_CONVS_EXCLUDED'):
        assert table in benchlib.wins.__doc__


def test_put_times_writes_two_keys_per_side_with_the_rounding():
    s = stats(parent=[10.04, 10.16, 10.26], fused=[3.333, 4.444, 5.555])
    row = benchlib.put_times({'kept': 1}, s, 1)
    assert row == {'kept': 1, 'parent_us': 10.2, 'parent_us_min_max': [10.0, 10.3], 'fused_us': 4.4,
                   'fused_us_min_max': [3.3, 5.6]}
    assert benchlib.put_times({}, s, 2) == {'parent_us': 10.16, 'parent_us_min_max': [10.04, 10.26], 'fused_us': 4.44,
                                            'fused_us_min_max': [3.33, 5.55]}


def test_limit_is_the_larger_bound_in_us_and_names_it():
    """The two classes of tools/bench_conv3x3_nchw.py with its formulas as literals; both are bound
    by compute (its recorded profile says so too: 17.07 and 16.21 us), so the bandwidth side is taken
    from tools/bench_conv1x1.py's 64 -> 64 @ 38912 class, 4.05 us of FLOPs under 4.98 us of bytes."""
    n = 2
    c, h, w = 512, 19, 32
    flops, nbytes = 2.0 * 16 * n * c * c * ((h + 1) // 2) * ((w + 1) // 2), 4.0 * (2 * n * c * h * w + 9 * c * c)
    assert (flops, nbytes) == (2684354560.0, 14417920.0)
    us, which = benchlib.limit(flops, nbytes)
    assert which == 'compute' and us == pytest.approx(2684354560.0 / 157.3e12 * 1e6, rel=1e-12) and round(us, 2) == 17.07
    c, h, w = 64, 152, 256
    flops, nbytes = 2.0 * 16 * n * c * c * ((h + 1) // 2) * ((w + 1) // 2), 4.0 * (2 * n * c * h * w + 9 * c * c)
    assert (flops, nbytes) == (2550136832.0, 39993344.0)
    us, which = benchlib.limit(flops, nbytes)
    assert which == 'compute' and round(us, 2) == 16.21 and us > nbytes / 8.0e12 * 1e6
    cin, cout, hw = 64, 64, 38912
    flops, nbytes = 2.0 * n * cin * cout * hw, 4.0 * (n * hw * (cin + cout) + cin * cout)
    assert (flops, nbytes) == (637534208.0, 39862272.0)
    us, which = benchlib.limit(flops, nbytes)
    assert which == 'bandwidth' and us == pytest.approx(39862272.0 / 8.0e12 * 1e6, rel=1e-12) and round(us, 2) == 4.98
    assert (benchlib.PEAK_FLOPS, benchlib.PEAK_BYTES) == (157.3e12, 8.0e12)


def test_max_rel_diff_over_tensors_and_nested_lists():
    import torch
    a, b = torch.tensor([1.0, -4.0]), torch.tensor([1.5, -4.0])
    assert benchlib.max_rel_diff(a, b) == 0.125
    assert benchlib.max_rel_diff([a, a], [a, b]) == 0.125
    assert benchlib.max_rel_diff(([a], [a, 2 * a]), ([a], [b, 2 * a])) == 0.125


# ------------------------------------------------------------------------- the tools that use it
@pytest.fixture(scope='module')
def help_runs():
    """Every tool imported and then run with --help, each in a process of its own without a device;
    started together, since each one spends its time importing torch."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    code = ('import sys, runpy; sys.argv = [{0!r}, "--help"]; import {1}; '
            'assert not __import__("torch").cuda.is_initialized(); runpy.run_path({0!r}, run_name="__main__")')
    procs = {t: subprocess.Popen([sys.executable, '-c', code.format(os.path.join(TOOLS, t + '.py'), t)], cwd=TOOLS,
                                 env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for t in CONVERTED}
    return {t: p.communicate() + (p.returncode,) for t, p in procs.items()}


@pytest.mark.parametrize('tool', CONVERTED)
def test_tool_imports_and_prints_its_help_without_a_device(help_runs, tool):
    out, err, code = help_runs[tool]
    assert code == 0, err[-2000:]
    assert 'usage:' in out


def test_no_tool_keeps_a_timer_or_a_counter_of_its_own():
    own = re.compile(r'^\s*def (time_calls|count_launches|count_syncs)\b', re.M)
    for name in sorted(os.listdir(TOOLS)):
        if not name.endswith('.py') or name == 'benchlib.py':
            continue
        text = open(os.path.join(TOOLS, name)).read()
        assert not own.search(text), name
        if name not in OWN_EVENT_PAIR:
            assert 'torch.cuda.Event' not in text and 'elapsed_time' not in text, name
    assert len(own.findall(open(os.path.join(TOOLS, 'benchlib.py')).read())) == 3
