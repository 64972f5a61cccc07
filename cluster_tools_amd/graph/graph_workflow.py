"""GraphWorkflow (reference: cluster_tools/graph/graph_workflow.py): the same parameters
(input_path / input_key / graph_path / output_key / n_scales), the same n5 / zarr check of the
input path and the same task chain InitialSubGraphs -> MergeSubGraphs (scales 1 .. n_scales - 1,
then the complete graph) -> MapEdgeIds, writing the region adjacency graph of a label volume --
nodes, edges and the voxel faces per edge -- to graph_path:output_key (the layout:
merge_sub_graphs.py).

The graph has the semantics of the reference's final graph as its test states them
(test/graph/test_graph.py:95-115: nodes and edges equal to nifty's gridRag); nifty is not
available here, so that parity is stated, not executed.  It is computed from the whole volume in
one device pass (cc_region_graph).  The reference's per-block sub-graphs (s<scale>/sub_graphs/
nodes, edges, edge_ids) are not produced: nifty's later stages are their only readers.  The
MergeSubGraphs tasks of the scales >= 1 and MapEdgeIds therefore write their logs only, and
n_scales changes nothing in the result.  target must be 'local'."""
from cluster_tools_amd.luigi_compat import Parameter, IntParameter
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.graph import initial_sub_graphs as initial_tasks
from cluster_tools_amd.graph import merge_sub_graphs as merge_tasks
from cluster_tools_amd.graph import map_edge_ids as map_tasks


class GraphWorkflow(WorkflowBase):
    input_path = Parameter()
    input_key = Parameter()
    graph_path = Parameter()
    output_key = Parameter()
    n_scales = IntParameter(default=1)

    # as the reference: n5 / zarr input labels only
    def _check_input(self):
        ending = self.input_path.split('.')[-1]
        assert ending.lower() in ('zr', 'zarr', 'n5'), "Only support n5 and zarr files, not %s" % ending

    def requires(self):
        self._check_input()
        common = dict(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir)
        initial_task = getattr(initial_tasks, self._get_task_name('InitialSubGraphs'))
        dep = initial_task(input_path=self.input_path, input_key=self.input_key, graph_path=self.graph_path,
                           dependency=self.dependency, **common)
        merge_task = getattr(merge_tasks, self._get_task_name('MergeSubGraphs'))
        for scale in range(1, self.n_scales):
            dep = merge_task(graph_path=self.graph_path, output_key='s%i/sub_graphs' % scale, scale=scale,
                             merge_complete_graph=False, dependency=dep, **common)
        dep = merge_task(graph_path=self.graph_path, output_key=self.output_key, scale=self.n_scales - 1,
                         merge_complete_graph=True, dependency=dep, **common)
        map_task = getattr(map_tasks, self._get_task_name('MapEdgeIds'))
        dep = map_task(graph_path=self.graph_path, input_key=self.output_key, scale=self.n_scales - 1,
                       dependency=dep, **common)
        return dep

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'initial_sub_graphs': initial_tasks.InitialSubGraphsLocal.default_task_config(),
                        'merge_sub_graphs': merge_tasks.MergeSubGraphsLocal.default_task_config(),
                        'map_edge_ids': map_tasks.MapEdgeIdsLocal.default_task_config()})
        return configs
