"""SizeFilterWorkflow (reference: cluster_tools/postprocess/postprocess_workflow.py:24-110): the
same parameters and task chain FindUniques(return_counts) -> SizeFilterBlocks ->
BackgroundSizeFilter, with the reference's tmp artefacts and logs.  relabel=True: the reference
chains a RelabelWorkflow (three more passes over the volume) behind the filter; here the
BackgroundSizeFilter job filters and relabels in one device call and writes the
`relabel_size_filter` assignment table and the new `maxId` itself.  hmap_path != '' (the
reference's FillingSizeFilter, a watershed fill) is not available.  target must be 'local'.

ConnectedComponentsWorkflow (reference :294-338) and SizeFilterAndGraphWatershedWorkflow (reference
:341-430) clean a node labelling up on the region graph, with the reference's parameters and task
chains: GraphConnectedComponents [-> Write, identifier 'graph-connected-components'], and
FindUniques(return_counts) -> SizeFilterBlocks(size_threshold | target_number) ->
GraphWatershedAssignments(filter_nodes_path = <tmp>/discard_ids.npy) [-> Write, identifier
'size-filter-graph-ws'].  The Write task runs when output_key is given and paints `fragments_key`
of `path` with the new assignments.  The reference passes prefix='size-filter-and-graph-watershed'
to FindUniques, which only renames that task's log and artefacts; FindUniques here has no prefix and
is chained as it is, so a SizeFilterWorkflow in the same tmp_folder shares its artefact names."""
import os

from cluster_tools_amd.luigi_compat import Parameter, IntParameter, BoolParameter
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.relabel import find_uniques as unique_tasks
from cluster_tools_amd.postprocess import size_filter_blocks as size_filter_tasks
from cluster_tools_amd.postprocess import background_size_filter as bg_tasks
from cluster_tools_amd.postprocess import graph_watershed_assignments as gws_tasks
from cluster_tools_amd.postprocess import graph_connected_components as cc_tasks
from cluster_tools_amd.write import write as write_tasks


class SizeFilterWorkflow(WorkflowBase):
    input_path = Parameter()
    input_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    size_threshold = IntParameter()
    hmap_path = Parameter(default='')
    hmap_key = Parameter(default='')
    relabel = BoolParameter(default=True)
    preserve_zeros = BoolParameter(default=False)

    def requires(self):
        if self.hmap_path != '':
            raise NotImplementedError('hmap_path: the filling size filter (FillingSizeFilter) is not available '
                                      'on the MI355X path')
        assert self.hmap_key == ''
        un_task = getattr(unique_tasks, self._get_task_name('FindUniques'))
        dep = un_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                      input_path=self.input_path, input_key=self.input_key, return_counts=True,
                      dependency=self.dependency)
        sf_task = getattr(size_filter_tasks, self._get_task_name('SizeFilterBlocks'))
        dep = sf_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                      input_path=self.input_path, input_key=self.input_key,
                      size_threshold=self.size_threshold, dependency=dep)
        filter_task = getattr(bg_tasks, self._get_task_name('BackgroundSizeFilter'))
        dep = filter_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                          input_path=self.input_path, input_key=self.input_key,
                          output_path=self.output_path, output_key=self.output_key,
                          relabel=self.relabel, assignment_key='relabel_size_filter', dependency=dep)
        return dep

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'find_uniques': unique_tasks.FindUniquesLocal.default_task_config(),
                        'size_filter_blocks': size_filter_tasks.SizeFilterBlocksLocal.default_task_config(),
                        'background_size_filter': bg_tasks.BackgroundSizeFilterLocal.default_task_config()})
        return configs


class ConnectedComponentsWorkflow(WorkflowBase):
    problem_path = Parameter()
    graph_key = Parameter()
    assignment_path = Parameter()
    assignment_key = Parameter()
    output_path = Parameter()
    assignment_out_key = Parameter()
    output_key = Parameter(default='')
    path = Parameter(default='')
    fragments_key = Parameter(default='')

    def requires(self):
        cc_task = getattr(cc_tasks, self._get_task_name('GraphConnectedComponents'))
        dep = cc_task(max_jobs=self.max_jobs, tmp_folder=self.tmp_folder, config_dir=self.config_dir,
                      problem_path=self.problem_path, graph_key=self.graph_key,
                      assignment_path=self.assignment_path, assignment_key=self.assignment_key,
                      output_path=self.output_path, output_key=self.assignment_out_key, dependency=self.dependency)
        if self.output_key != '':
            assert self.fragments_key != '' and self.path != ''
            write_task = getattr(write_tasks, self._get_task_name('Write'))
            dep = write_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                             dependency=dep, input_path=self.path, input_key=self.fragments_key,
                             output_path=self.output_path, output_key=self.output_key,
                             assignment_path=self.output_path, assignment_key=self.assignment_out_key,
                             identifier='graph-connected-components')
        return dep

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'graph_connected_components': cc_tasks.GraphConnectedComponentsLocal.default_task_config(),
                        'write': write_tasks.WriteLocal.default_task_config()})
        return configs


class SizeFilterAndGraphWatershedWorkflow(WorkflowBase):
    problem_path = Parameter()
    graph_key = Parameter()
    features_key = Parameter()
    path = Parameter()
    segmentation_key = Parameter()          # the merged segmentation, whose segment sizes are counted
    fragments_key = Parameter(default='')   # the fragments under it
    assignment_key = Parameter()            # the fragment-to-segment assignment
    size_threshold = IntParameter(default=None)
    target_number = IntParameter(default=None)
    relabel = BoolParameter(default=False)
    from_costs = BoolParameter(default=False)
    output_path = Parameter()
    assignment_out_key = Parameter()
    output_key = Parameter(default='')

    def find_sizes(self, dep):
        un_task = getattr(unique_tasks, self._get_task_name('FindUniques'))
        dep = un_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                      input_path=self.path, input_key=self.segmentation_key, return_counts=True, dependency=dep)
        sf_task = getattr(size_filter_tasks, self._get_task_name('SizeFilterBlocks'))
        return sf_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                       input_path=self.path, input_key=self.segmentation_key, size_threshold=self.size_threshold,
                       target_number=self.target_number, dependency=dep)

    def requires(self):
        assert (self.size_threshold is None) != (self.target_number is None)
        dep = self.find_sizes(self.dependency)
        filter_path = os.path.join(self.tmp_folder, 'discard_ids.npy')
        gws_task = getattr(gws_tasks, self._get_task_name('GraphWatershedAssignments'))
        dep = gws_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir, dependency=dep,
                       problem_path=self.problem_path, graph_key=self.graph_key, features_key=self.features_key,
                       assignment_path=self.path, assignment_key=self.assignment_key,
                       output_path=self.output_path, output_key=self.assignment_out_key,
                       filter_nodes_path=filter_path, relabel=self.relabel, from_costs=self.from_costs)
        if self.output_key != '':
            assert self.fragments_key != ''
            write_task = getattr(write_tasks, self._get_task_name('Write'))
            dep = write_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                             dependency=dep, input_path=self.path, input_key=self.fragments_key,
                             output_path=self.output_path, output_key=self.output_key,
                             assignment_path=self.output_path, assignment_key=self.assignment_out_key,
                             identifier='size-filter-graph-ws')
        return dep

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'size_filter_blocks': size_filter_tasks.SizeFilterBlocksLocal.default_task_config(),
                        'graph_watershed_assignments': gws_tasks.GraphWatershedAssignmentsLocal.default_task_config(),
                        'write': write_tasks.WriteLocal.default_task_config()})
        return configs
