"""ProblemWorkflow and MulticutSegmentationWorkflow (reference: cluster_tools/workflows.py:28-107,
110-232), the reference's main entry point: supervoxels -> region adjacency graph -> edge features
-> edge costs -> multicut -> segmentation.  The parameters are the reference's, and so are the
hard-coded keys of the problem file: the graph under s0/graph, the edge features under features,
the costs under s0/costs.

ProblemWorkflow chains GraphWorkflow (n_scales = 1) -> EdgeFeaturesWorkflow -> EdgeCostsWorkflow
(when compute_costs).  MulticutSegmentationWorkflow puts MulticutWorkflow and the Write task
(identifier 'multicut') behind it; with output_key '' the segmentation is not written, as in the
reference.  What is not built raises NotImplementedError:
  * skip_ws must be True: there is no WatershedWorkflow, the supervoxels ws_path:ws_key are made
    beforehand (the Watershed task, watershed/watershed.py) and must exist;
  * agglomerate_ws, two_pass_ws (options of that workflow) and sanity_checks
    (CheckSubGraphsWorkflow: there are no per-block sub-graphs to check) must be False;
  * n_scales must be 0 (multicut/multicut_workflow.py), rf_path '' (costs/costs_workflow.py).
target must be 'local'.

AgglomerativeClusteringWorkflow (reference: workflows.py:326-357) is the second entry point on the
same problem file: ProblemWorkflow without the costs, then the AgglomerativeClustering task on the
edge features (problem_path:features) up to `threshold`, then Write (identifier
'agglomerative_clustering').  The same settings are not built."""
import os

from cluster_tools_amd.luigi_compat import Parameter, IntParameter, FloatParameter, BoolParameter, DictParameter
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.graph import GraphWorkflow
from cluster_tools_amd.features import EdgeFeaturesWorkflow
from cluster_tools_amd.costs import EdgeCostsWorkflow
from cluster_tools_amd.multicut import MulticutWorkflow
from cluster_tools_amd.agglomerative_clustering import agglomerative_clustering as agglomerate_tasks
from cluster_tools_amd.write import write as write_tasks


class ProblemWorkflow(WorkflowBase):
    input_path = Parameter()
    input_key = Parameter()
    ws_path = Parameter()
    ws_key = Parameter()
    problem_path = Parameter()
    rf_path = Parameter(default='')
    node_label_dict = DictParameter(default={})
    max_jobs_merge = IntParameter(default=1)
    compute_costs = BoolParameter(default=True)
    sanity_checks = BoolParameter(default=False)

    graph_key = 's0/graph'
    features_key = 'features'
    costs_key = 's0/costs'

    def requires(self):
        if self.sanity_checks:
            raise NotImplementedError('sanity_checks: there are no per-block sub-graphs to check; it must be False')
        common = dict(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir, target=self.target)
        dep = GraphWorkflow(dependency=self.dependency, input_path=self.ws_path, input_key=self.ws_key,
                            graph_path=self.problem_path, output_key=self.graph_key, n_scales=1, **common)
        dep = EdgeFeaturesWorkflow(dependency=dep, input_path=self.input_path, input_key=self.input_key,
                                   labels_path=self.ws_path, labels_key=self.ws_key, graph_path=self.problem_path,
                                   graph_key=self.graph_key, output_path=self.problem_path,
                                   output_key=self.features_key, max_jobs_merge=self.max_jobs_merge, **common)
        if self.compute_costs:
            dep = EdgeCostsWorkflow(dependency=dep, features_path=self.problem_path, features_key=self.features_key,
                                    output_path=self.problem_path, output_key=self.costs_key,
                                    node_label_dict=self.node_label_dict, seg_path=self.ws_path, seg_key=self.ws_key,
                                    rf_path=self.rf_path, **common)
        return dep

    @staticmethod
    def get_config():
        return {**GraphWorkflow.get_config(), **EdgeFeaturesWorkflow.get_config(), **EdgeCostsWorkflow.get_config()}


class SegmentationWorkflowBase(WorkflowBase):
    input_path = Parameter()
    input_key = Parameter()
    ws_path = Parameter()                 # the supervoxels
    ws_key = Parameter()
    problem_path = Parameter()            # graph, edge features, costs
    node_labels_key = Parameter()         # the node labelling, in output_path
    output_path = Parameter()
    output_key = Parameter()
    mask_path = Parameter(default='')
    mask_key = Parameter(default='')
    rf_path = Parameter(default='')
    node_label_dict = DictParameter(default={})
    max_jobs_merge = IntParameter(default=1)
    skip_ws = BoolParameter(default=False)
    agglomerate_ws = BoolParameter(default=False)
    two_pass_ws = BoolParameter(default=False)
    sanity_checks = BoolParameter(default=False)

    graph_key = 's0/graph'
    features_key = 'features'
    costs_key = 's0/costs'

    def _watershed_tasks(self):
        if not self.skip_ws:
            raise NotImplementedError('skip_ws=False: WatershedWorkflow is not built; make the supervoxels with the '
                                      'Watershed task first and pass skip_ws=True')
        for name in ('agglomerate_ws', 'two_pass_ws'):
            if getattr(self, name):
                raise NotImplementedError('%s is an option of WatershedWorkflow, which is not built; it must be False'
                                          % name)
        assert os.path.exists(os.path.join(self.ws_path, self.ws_key)), '%s:%s' % (self.ws_path, self.ws_key)
        return self.dependency

    def _problem_tasks(self, dep, compute_costs):
        return ProblemWorkflow(tmp_folder=self.tmp_folder, config_dir=self.config_dir, max_jobs=self.max_jobs,
                               target=self.target, dependency=dep, input_path=self.input_path,
                               input_key=self.input_key, ws_path=self.ws_path, ws_key=self.ws_key,
                               problem_path=self.problem_path, rf_path=self.rf_path,
                               node_label_dict=self.node_label_dict, max_jobs_merge=self.max_jobs_merge,
                               compute_costs=compute_costs, sanity_checks=self.sanity_checks)

    def _write_tasks(self, dep, identifier):
        if self.output_key == '':
            return dep
        write_task = getattr(write_tasks, self._get_task_name('Write'))
        return write_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                          dependency=dep, input_path=self.ws_path, input_key=self.ws_key,
                          output_path=self.output_path, output_key=self.output_key,
                          assignment_path=self.output_path, assignment_key=self.node_labels_key,
                          identifier=identifier)

    @staticmethod
    def get_config():
        return ProblemWorkflow.get_config()


class MulticutSegmentationWorkflow(SegmentationWorkflowBase):
    max_jobs_multicut = IntParameter(default=1)
    n_scales = IntParameter()

    def _multicut_tasks(self, dep):
        return MulticutWorkflow(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs_multicut,
                                config_dir=self.config_dir, target=self.target, dependency=dep,
                                problem_path=self.problem_path, n_scales=self.n_scales,
                                assignment_path=self.output_path, assignment_key=self.node_labels_key)

    def requires(self):
        dep = self._watershed_tasks()
        dep = self._problem_tasks(dep, compute_costs=True)
        dep = self._multicut_tasks(dep)
        return self._write_tasks(dep, 'multicut')

    @staticmethod
    def get_config():
        config = SegmentationWorkflowBase.get_config()
        config.update(MulticutWorkflow.get_config())
        config.update({'write': write_tasks.WriteLocal.default_task_config()})
        return config


class AgglomerativeClusteringWorkflow(SegmentationWorkflowBase):
    threshold = FloatParameter()

    def _agglomerate_task(self, dep):
        agglomerate_task = getattr(agglomerate_tasks, self._get_task_name('AgglomerativeClustering'))
        return agglomerate_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                                problem_path=self.problem_path, assignment_path=self.output_path,
                                assignment_key=self.node_labels_key, features_path=self.problem_path,
                                features_key=self.features_key, threshold=self.threshold, dependency=dep)

    def requires(self):
        dep = self._watershed_tasks()
        dep = self._problem_tasks(dep, compute_costs=False)
        dep = self._agglomerate_task(dep)
        return self._write_tasks(dep, 'agglomerative_clustering')

    @staticmethod
    def get_config():
        config = SegmentationWorkflowBase.get_config()
        config.update({'agglomerative_clustering': agglomerate_tasks.AgglomerativeClusteringLocal.default_task_config()})
        return config
