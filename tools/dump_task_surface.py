#! /usr/bin/python
"""The drop-in surface of every *Local task class of cluster_tools_amd, as JSON: task_name,
allow_retry, the parameters with their defaults and default_task_config().

    python tools/dump_task_surface.py > tests/golden/task_surface.json

tests/test_task_framework.py rebuilds the same dict from the current classes and compares it with
the committed dump, so regenerate the dump only where a task's surface is meant to change.

The dump is split over files.  A module of tasks added later is listed in ADDENDA and dumped into a
file of its own, which tests/test_task_surface_addenda.py compares in the same way:

    python tools/dump_task_surface.py watershed > tests/golden/task_surface_watershed.json

task_surface() covers every module that no addendum claims, so a new *Local task fails the first
comparison until it is either dumped there or claimed by an addendum; every task is in exactly one
file.
"""
import importlib
import inspect
import json
import os
import pkgutil
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cluster_tools_amd  # noqa: E402
from cluster_tools_amd.cluster_tasks import BaseClusterTask  # noqa: E402
from cluster_tools_amd.luigi_compat import Parameter  # noqa: E402


def _default(param):
    d = getattr(param, 'default', getattr(param, '_default', None))
    if d is None or isinstance(d, (bool, int, float, str)):
        return d
    if isinstance(d, (list, tuple)):
        return list(d)
    return type(d).__name__            # a task instance (dependency = DummyTask())


# addendum name -> the modules whose tasks tests/golden/task_surface_<name>.json holds
ADDENDA = {'watershed': ('cluster_tools_amd.watershed.watershed',),
           'multicut': ('cluster_tools_amd.costs.probs_to_costs', 'cluster_tools_amd.multicut.solve_global'),
           'agglomerative_clustering': ('cluster_tools_amd.agglomerative_clustering.agglomerative_clustering',),
           'graph_postprocess': ('cluster_tools_amd.postprocess.graph_connected_components',
                                 'cluster_tools_amd.postprocess.graph_watershed_assignments')}


def task_surface(addendum=None):
    """The surface of the tasks of the addendum's modules; None: of every module no addendum claims."""
    claimed = {m for mods in ADDENDA.values() for m in mods}
    surface = {}
    for info in pkgutil.walk_packages(cluster_tools_amd.__path__, 'cluster_tools_amd.'):
        if (info.name in claimed) if addendum is None else (info.name not in ADDENDA[addendum]):
            continue
        module = importlib.import_module(info.name)
        for name, klass in inspect.getmembers(module, inspect.isclass):
            if not (name.endswith('Local') and issubclass(klass, BaseClusterTask)
                    and klass.__module__ == info.name):
                continue
            params = {}
            for k in reversed(klass.__mro__):
                params.update({n: _default(p) for n, p in vars(k).items() if isinstance(p, Parameter)})
            surface['%s.%s' % (info.name, name)] = {
                'task_name': klass.task_name, 'allow_retry': klass.allow_retry,
                'parameters': dict(sorted(params.items())),
                'default_task_config': klass.default_task_config()}
    return dict(sorted(surface.items()))


if __name__ == '__main__':
    json.dump(task_surface(sys.argv[1] if len(sys.argv) > 1 else None), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write('\n')
