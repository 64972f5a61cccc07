#! /usr/bin/python
"""MapEdgeIds task (reference: cluster_tools/graph/map_edge_ids.py).

Same task surface as the reference (map_edge_ids.py:19-76): parameters graph_path / input_key /
scale / dependency, allow_retry = False, the log target <tmp>/map_edge_ids_s<scale>.log.  The
reference's job (nifty's mapEdgeIdsForAllBlocks, :103-117) gives every per-block sub-graph the
ids its edges have in the complete graph (dataset s<scale>/sub_graphs/edge_ids).  The per-block
sub-graphs are not produced here (see initial_sub_graphs.py), so there is nothing to map: the
task writes its log only, with one line that says so.  The id of an edge in the complete graph is
its row in graph_path:input_key/edges.
"""
import os

from cluster_tools_amd.luigi_compat import Task, Parameter, IntParameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask


class MapEdgeIdsBase(Task):
    task_name = 'map_edge_ids'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    graph_path = Parameter()
    input_key = Parameter()
    scale = IntParameter()
    dependency = TaskParameter(default=DummyTask())

    def run_impl(self):
        self._write_log('per-block sub-graphs are not produced, no edge ids to map at scale %i: the id of an edge '
                        'is its row in %s:%s/edges' % (self.scale, self.graph_path, self.input_key))

    def output(self):
        return self.prefixed_output('s%i' % self.scale)


class MapEdgeIdsLocal(MapEdgeIdsBase, LocalTask):
    pass
