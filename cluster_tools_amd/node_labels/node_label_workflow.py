"""NodeLabelWorkflow (reference: cluster_tools/node_labels/node_label_workflow.py): the same
parameters (ws_path / ws_key / input_path / input_key / output_path / output_key / prefix /
max_overlap / ignore_label / serialize_counts), the same temporary key label_overlaps_<prefix> and
the same task chain BlockNodeLabels -> MergeNodeLabels: which object of the label volume
input_path:input_key every node (id) of the ws volume belongs to, written to
output_path:output_key (the layouts: merge_node_labels.py).  The overlaps are counted over the
whole volume in one device pass (cc_label_overlaps).  target must be 'local'."""
from cluster_tools_amd.luigi_compat import Parameter, IntParameter, BoolParameter
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.node_labels import block_node_labels as label_tasks
from cluster_tools_amd.node_labels import merge_node_labels as merge_tasks


class NodeLabelWorkflow(WorkflowBase):
    ws_path = Parameter()
    ws_key = Parameter()
    input_path = Parameter()
    input_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    prefix = Parameter(default='')
    max_overlap = BoolParameter(default=True)
    ignore_label = IntParameter(default=None)
    serialize_counts = BoolParameter(default=False)

    def requires(self):
        common = dict(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir)
        label_task = getattr(label_tasks, self._get_task_name('BlockNodeLabels'))
        tmp_key = 'label_overlaps_%s' % self.prefix
        dep = label_task(dependency=self.dependency, ws_path=self.ws_path, ws_key=self.ws_key,
                         input_path=self.input_path, input_key=self.input_key, output_path=self.output_path,
                         output_key=tmp_key, ignore_label=self.ignore_label, prefix=self.prefix, **common)
        merge_task = getattr(merge_tasks, self._get_task_name('MergeNodeLabels'))
        dep = merge_task(dependency=dep, input_path=self.output_path, input_key=tmp_key,
                         output_path=self.output_path, output_key=self.output_key, max_overlap=self.max_overlap,
                         ignore_label=self.ignore_label, serialize_counts=self.serialize_counts,
                         prefix=self.prefix, **common)
        return dep

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'block_node_labels': label_tasks.BlockNodeLabelsLocal.default_task_config(),
                        'merge_node_labels': merge_tasks.MergeNodeLabelsLocal.default_task_config()})
        return configs
