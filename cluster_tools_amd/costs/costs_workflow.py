"""EdgeCostsWorkflow (reference: cluster_tools/costs/costs_workflow.py): the same parameters
(features_path / features_key / output_path / output_key / node_label_dict / seg_path / seg_key /
rf_path) and get_config.  Without node labels the workflow is the ProbsToCosts task on column 0 of
the edge features; with node_label_dict = {mode: (path, key)} each label volume is first mapped to
the nodes of seg_path:seg_key by a NodeLabelWorkflow (max_overlap, no ignore label, prefix
cost_labels_<key>, output <key>_mapped beside the volume), as in the reference (:62-77).  rf_path
other than '' (edge probabilities from a random forest, the reference's Predict task) is not
built: NotImplementedError.  target must be 'local'."""
from cluster_tools_amd.luigi_compat import Parameter, DictParameter
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.costs import probs_to_costs as transform_tasks


class EdgeCostsWorkflow(WorkflowBase):
    features_path = Parameter()
    features_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    node_label_dict = DictParameter(default={})
    seg_path = Parameter(default=None)
    seg_key = Parameter(default=None)
    rf_path = Parameter(default='')

    def _map_node_labels(self, dep):
        from cluster_tools_amd.node_labels import NodeLabelWorkflow
        assert self.seg_path is not None and self.seg_key is not None
        mapped = {}
        for mode, (path, key) in dict(self.node_label_dict).items():
            out_key = '%s_mapped' % key
            dep = NodeLabelWorkflow(tmp_folder=self.tmp_folder, config_dir=self.config_dir, target=self.target,
                                    max_jobs=self.max_jobs, dependency=dep, ws_path=self.seg_path, ws_key=self.seg_key,
                                    input_path=path, input_key=key, prefix='cost_labels_%s' % '_'.join(key.split('/')),
                                    output_path=path, output_key=out_key, max_overlap=True, ignore_label=None)
            mapped[mode] = (path, out_key)
        return dep, mapped

    def requires(self):
        if self.rf_path != '':
            raise NotImplementedError("rf_path '%s': edge probabilities from a random forest are not built; "
                                      "rf_path must be ''" % self.rf_path)
        dep, mapped = self.dependency, {}
        if self.node_label_dict:
            dep, mapped = self._map_node_labels(dep)
        task = getattr(transform_tasks, self._get_task_name('ProbsToCosts'))
        return task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                    input_path=self.features_path, input_key=self.features_key, features_path=self.features_path,
                    features_key=self.features_key, output_path=self.output_path, output_key=self.output_key,
                    dependency=dep, node_label_dict=mapped)

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'probs_to_costs': transform_tasks.ProbsToCostsLocal.default_task_config()})
        return configs
