"""EdgeFeaturesWorkflow and RegionFeaturesWorkflow (reference:
cluster_tools/features/features_workflow.py).

EdgeFeaturesWorkflow (features_workflow.py:12-64): the same parameters (max_jobs_merge included),
the n5 / zarr check of the input and label paths, get_config and the task chain BlockEdgeFeatures
-> MergeEdgeFeatures, writing the float64 (n_edges, 10) table of per-edge statistics (mean,
variance, min, q10, q25, q50, q75, q90, max, count) for the edges of graph_path:graph_key, which
GraphWorkflow must have written from the same labels: of a 3-D boundary map, or, with `offsets` in
the block_edge_features task config, of a 4-D (C, Z, Y, X) affinity map.  Filter responses, the
per-block s0/sub_features and the costs and multicut stages are not built.

RegionFeaturesWorkflow: the same
parameters and task chain RegionFeatures -> MergeRegionFeatures, writing the (maxId + 1,
n_features) float32 table of per-id intensity features (count and mean; minimum and maximum when
the region_features task config asks for them) of an input volume over a label volume.
number_of_labels = maxId + 1 is read from the label dataset's attributes in requires(), as the
reference does, so the labels must have been written (with their maxId) before the workflow is
instantiated into a task graph.  target must be 'local'."""
from cluster_tools_amd.luigi_compat import Parameter, IntParameter
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.utils import volume_utils as vu
from cluster_tools_amd.features import region_features as feat_tasks
from cluster_tools_amd.features import merge_region_features as merge_tasks
from cluster_tools_amd.features import block_edge_features as edge_tasks
from cluster_tools_amd.features import merge_edge_features as merge_edge_tasks


class EdgeFeaturesWorkflow(WorkflowBase):
    input_path = Parameter()
    input_key = Parameter()
    labels_path = Parameter()
    labels_key = Parameter()
    graph_path = Parameter()
    graph_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    max_jobs_merge = IntParameter(default=1)

    # only n5 / zarr inputs, as the reference
    @staticmethod
    def _check_input(path):
        ending = path.split('.')[-1]
        assert ending.lower() in ('zr', 'zarr', 'n5'), "Only support n5 and zarr files, not %s" % ending

    def requires(self):
        self._check_input(self.input_path)
        self._check_input(self.labels_path)
        feat_task = getattr(edge_tasks, self._get_task_name('BlockEdgeFeatures'))
        dep = feat_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                        input_path=self.input_path, input_key=self.input_key, labels_path=self.labels_path,
                        labels_key=self.labels_key, graph_path=self.graph_path, output_path=self.output_path,
                        dependency=self.dependency)
        merge_task = getattr(merge_edge_tasks, self._get_task_name('MergeEdgeFeatures'))
        dep = merge_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs_merge, config_dir=self.config_dir,
                         graph_path=self.graph_path, graph_key=self.graph_key, output_path=self.output_path,
                         output_key=self.output_key, dependency=dep)
        return dep

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'block_edge_features': edge_tasks.BlockEdgeFeaturesLocal.default_task_config(),
                        'merge_edge_features': merge_edge_tasks.MergeEdgeFeaturesLocal.default_task_config()})
        return configs


class RegionFeaturesWorkflow(WorkflowBase):
    input_path = Parameter()
    input_key = Parameter()
    labels_path = Parameter()
    labels_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    prefix = Parameter(default='')
    max_jobs_merge = IntParameter(default=None)
    channel = IntParameter(default=None)

    def read_number_of_labels(self):
        with vu.file_reader(self.labels_path, 'r') as f:
            max_id = f[self.labels_key].attrs.get('maxId', None)
        if max_id is None:
            raise ValueError("%s:%s has no 'maxId' attribute: the feature table has maxId + 1 rows (the "
                             "connected-components and size-filter jobs write it)" % (self.labels_path, self.labels_key))
        return int(max_id) + 1

    def requires(self):
        feat_task = getattr(feat_tasks, self._get_task_name('RegionFeatures'))
        dep = feat_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                        input_path=self.input_path, input_key=self.input_key, labels_path=self.labels_path,
                        labels_key=self.labels_key, prefix=self.prefix, channel=self.channel,
                        dependency=self.dependency)
        merge_task = getattr(merge_tasks, self._get_task_name('MergeRegionFeatures'))
        max_jobs_merge = self.max_jobs if self.max_jobs_merge is None else self.max_jobs_merge
        dep = merge_task(tmp_folder=self.tmp_folder, max_jobs=max_jobs_merge, config_dir=self.config_dir,
                         output_path=self.output_path, output_key=self.output_key,
                         number_of_labels=self.read_number_of_labels(), prefix=self.prefix, dependency=dep)
        return dep

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'region_features': feat_tasks.RegionFeaturesLocal.default_task_config(),
                        'merge_region_features': merge_tasks.MergeRegionFeaturesLocal.default_task_config()})
        return configs
