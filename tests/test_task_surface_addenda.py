"""The addenda of the committed task surface (tools/dump_task_surface.py: ADDENDA): the tasks of
modules added after tests/golden/task_surface.json, each module's dump in a file of its own, compared
as tests/test_task_framework.py compares the first file.  Every *Local task of the package is in
exactly one of the files."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location('dump_task_surface',
                                                  os.path.join(ROOT, 'tools', 'dump_task_surface.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _golden(name):
    with open(os.path.join(ROOT, 'tests', 'golden', name)) as f:
        return json.load(f)


def test_addenda_are_the_committed_ones():
    mod = _tool()
    assert mod.ADDENDA
    for name in mod.ADDENDA:
        want = _golden('task_surface_%s.json' % name)
        got = json.loads(json.dumps(mod.task_surface(name)))
        assert sorted(got) == sorted(want) and want, name
        for task in want:
            assert got[task] == want[task], task


def test_watershed_task_is_in_its_addendum():
    want = _golden('task_surface_watershed.json')
    assert list(want) == ['cluster_tools_amd.watershed.watershed.WatershedLocal']
    task = want['cluster_tools_amd.watershed.watershed.WatershedLocal']
    assert task['task_name'] == 'watershed' and task['allow_retry'] is False
    assert task['default_task_config']['size_filter'] == 25 and task['default_task_config']['alpha'] == 0.8


def test_every_task_is_in_exactly_one_file():
    import importlib
    import inspect
    import pkgutil
    import cluster_tools_amd
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    mod = _tool()
    files = [mod.task_surface()] + [mod.task_surface(name) for name in mod.ADDENDA]
    names = [t for f in files for t in f]
    assert len(names) == len(set(names))
    found = set()
    for info in pkgutil.walk_packages(cluster_tools_amd.__path__, 'cluster_tools_amd.'):
        module = importlib.import_module(info.name)
        for name, klass in inspect.getmembers(module, inspect.isclass):
            if name.endswith('Local') and issubclass(klass, BaseClusterTask) and klass.__module__ == info.name:
                found.add('%s.%s' % (info.name, name))
    assert found == set(names)
