"""The reference's task/job contract on the cluster_tools_amd framework (CPU): job configs with
strided block lists, script copy + shebang, 'processed job' tokens, luigi targets, retries."""
import json
import os
import sys

import pytest

from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.cluster_tasks import DummyTask, BaseClusterTask, FailedJobsError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dummy_task  # noqa: E402


def _configs(tmp_path, retries=0):
    cfg = str(tmp_path / 'config')
    os.makedirs(cfg, exist_ok=True)
    g = BaseClusterTask.default_global_config()
    g.update({'block_shape': [4, 4, 4], 'max_num_retries': retries})
    with open(os.path.join(cfg, 'global.config'), 'w') as f:
        json.dump(g, f)
    return cfg


def test_jobs_run_and_targets(tmp_path):
    out = tmp_path / 'out'
    out.mkdir()
    t = _dummy_task.DummyStageLocal(tmp_folder=str(tmp_path / 'tmp'), config_dir=_configs(tmp_path), max_jobs=3,
                                    out_path=str(out), dependency=DummyTask())
    assert luigi.build([t], local_scheduler=True)
    assert sorted(os.listdir(out)) == sorted('block_%d' % b for b in range(10))
    tmp = tmp_path / 'tmp'
    assert (tmp / 'dummy_stage.log').exists() and (tmp / 'dummy_stage.py').exists()
    job0 = json.load(open(tmp / 'dummy_stage_job_0.config'))
    assert job0['block_list'] == [0, 3, 6, 9]                 # block_list[job_id::n_jobs]
    last = open(tmp / 'logs' / 'dummy_stage_2.log').read().strip().split('\n')[-1]
    assert last.endswith('processed job 2')
    assert t.complete()


def test_failure_without_retry_moves_log(tmp_path):
    out = tmp_path / 'out'
    out.mkdir()
    t = _dummy_task.DummyStageLocal(tmp_folder=str(tmp_path / 'tmp'), config_dir=_configs(tmp_path), max_jobs=2,
                                    out_path=str(out), fail_first='yes', dependency=DummyTask())
    t.make_dirs()
    with pytest.raises(FailedJobsError):
        t.run()
    assert (tmp_path / 'tmp' / 'dummy_stage_failed.log').exists()


def test_retry_recovers_failed_blocks(tmp_path):
    out = tmp_path / 'out'
    out.mkdir()
    t = _dummy_task.DummyStageLocal(tmp_folder=str(tmp_path / 'tmp'), config_dir=_configs(tmp_path, 2), max_jobs=4,
                                    out_path=str(out), fail_first='yes', dependency=DummyTask())
    # 2 of 4 jobs fail (jobs 1 and 3 own odd blocks first) -> 50% -> no retry (reference rule)
    t.make_dirs()
    with pytest.raises(FailedJobsError):
        t.run()


def test_workflow_rejects_other_targets():
    from cluster_tools_amd.thresholded_components import ThresholdedComponentsWorkflow
    w = ThresholdedComponentsWorkflow(tmp_folder='x', max_jobs=1, config_dir='x', target='slurm',
                                      input_path='x', input_key='x', output_path='x', output_key='x',
                                      assignment_key='x', threshold=0.5)
    with pytest.raises(NotImplementedError):
        w._get_task_name('BlockComponents')


def test_run_jobs_names_configs_and_logs(tmp_path):
    """run_jobs leaves what prepare / submit / wait / check_jobs left, with and without a job prefix."""
    for prefix, cfg_name, log_name, target in (
            ('', 'dummy_stage_job_%d.config', 'dummy_stage_%d.log', 'dummy_stage.log'),
            ('pre_fix', 'dummy_stage_job_pre_fix_%d.config', 'dummy_stage_pre_fix_%d.log', 'dummy_stage_pre_fix.log')):
        out = tmp_path / ('out_' + prefix)
        out.mkdir()
        tmp = tmp_path / ('tmp_' + prefix)
        t = _dummy_task.DummyStageLocal(tmp_folder=str(tmp), config_dir=_configs(tmp_path), max_jobs=2,
                                        out_path=str(out), prefix=prefix, dependency=DummyTask())
        assert luigi.build([t], local_scheduler=True)
        assert sorted(os.listdir(out)) == sorted('block_%d' % b for b in range(10))
        configs = sorted(f for f in os.listdir(tmp) if f.endswith('.config'))
        assert configs == [cfg_name % j for j in range(2)]
        assert json.load(open(tmp / (cfg_name % 1)))['block_list'] == [1, 3, 5, 7, 9]
        assert sorted(os.listdir(tmp / 'logs')) == [log_name % j for j in range(2)]
        for j in range(2):
            assert open(tmp / 'logs' / (log_name % j)).read().strip().endswith('processed job %d' % j)
        assert (tmp / target).exists() and t.complete()
        task_log = open(tmp / target).read()
        assert 'written config for 2 jobs' in task_log and 'dummy_stage finished successfully' in task_log


def test_requires_defaults_to_the_dependency():
    assert 'requires' not in vars(_dummy_task.DummyStageBase) and 'requires' not in vars(_dummy_task.DummyStageLocal)
    dep = DummyTask()
    t = _dummy_task.DummyStageLocal(tmp_folder='x', config_dir='x', max_jobs=1, out_path='x', dependency=dep)
    assert t.requires() is dep


def test_run_job_parses_the_job_id(tmp_path, monkeypatch):
    import cluster_tools_amd.utils.function_utils as fu
    for name, want in (('x_job_3.config', 3), ('x_job_pre_fix_12.config', 12)):
        path = str(tmp_path / name)
        open(path, 'w').close()
        calls = []
        monkeypatch.setattr(sys, 'argv', ['script.py', path])
        fu.run_job(lambda job_id, config_path: calls.append((job_id, config_path)))
        assert calls == [(want, path)]
    monkeypatch.setattr(sys, 'argv', ['script.py', str(tmp_path / 'missing_job_0.config')])
    with pytest.raises(AssertionError):
        fu.run_job(lambda job_id, config_path: pytest.fail('called for a missing config'))


def test_job_config_logs_the_prologue(tmp_path, capsys):
    import cluster_tools_amd.utils.function_utils as fu
    path = str(tmp_path / 'x_job_7.config')
    with open(path, 'w') as f:
        json.dump({'block_list': [1, 2], 'k': 'v'}, f)
    assert fu.job_config(7, path) == {'block_list': [1, 2], 'k': 'v'}
    fu.log_blocks_success([1, 2])
    lines = capsys.readouterr().out.split('\n')
    assert [ln.split(': ', 1)[1] for ln in lines[:-1]] == [
        'start processing job 7', 'reading config from %s' % path, 'processed block 1', 'processed block 2']
    assert lines[-1] == ''


def test_function_utils_imports_neither_numpy_nor_torch():
    import subprocess
    code = ('import sys; import cluster_tools_amd.utils.function_utils; '
            'print(sorted(m for m in ("numpy", "torch") if m in sys.modules))')
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, '-c', code], cwd=repo, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == '[]', out.stdout


def test_task_surface_is_the_committed_one():
    """task_name, allow_retry, parameters with defaults and default_task_config() of every *Local task:
    the drop-in surface, dumped by tools/dump_task_surface.py into tests/golden/task_surface.json."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('dump_task_surface',
                                                  os.path.join(root, 'tools', 'dump_task_surface.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(root, 'tests', 'golden', 'task_surface.json')) as f:
        want = json.load(f)
    got = json.loads(json.dumps(mod.task_surface()))
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
