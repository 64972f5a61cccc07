"""MorphologyWorkflow (reference: cluster_tools/morphology/morphology_workflow.py:11-56): the same
parameters and task chain BlockMorphology -> MergeMorphology, writing the (maxId + 1, 11) float64
table (id, size, centre of mass, bounding-box minimum and inclusive maximum) that the reference's
skeleton, mesh, object-distance and region-centre workflows read.  number_of_labels = maxId + 1
is read from the input dataset's attributes in requires(), as the reference does, so the labels
must have been written (with their maxId) before the workflow is instantiated into a task graph.
RegionCentersWorkflow (a per-object Euclidean distance transform) is not available.  target must
be 'local'."""
from cluster_tools_amd.luigi_compat import Parameter, IntParameter
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.utils import volume_utils as vu
from cluster_tools_amd.morphology import block_morphology as block_tasks
from cluster_tools_amd.morphology import merge_morphology as merge_tasks


class MorphologyWorkflow(WorkflowBase):
    input_path = Parameter()
    input_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    max_jobs_merge = IntParameter(default=None)
    prefix = Parameter(default='')

    def _number_of_labels(self):
        with vu.file_reader(self.input_path, 'r') as f:
            max_id = f[self.input_key].attrs.get('maxId', None)
        if max_id is None:
            raise ValueError("%s:%s has no 'maxId' attribute: the morphology table has maxId + 1 rows (the "
                             "connected-components and size-filter jobs write it)" % (self.input_path, self.input_key))
        return int(max_id) + 1

    def requires(self):
        block_task = getattr(block_tasks, self._get_task_name('BlockMorphology'))
        tmp_key = 'morphology_%s' % self.prefix
        dep = block_task(max_jobs=self.max_jobs, tmp_folder=self.tmp_folder, config_dir=self.config_dir,
                         dependency=self.dependency, input_path=self.input_path, input_key=self.input_key,
                         output_path=self.output_path, output_key=tmp_key, prefix=self.prefix)
        merge_task = getattr(merge_tasks, self._get_task_name('MergeMorphology'))
        max_jobs_merge = self.max_jobs if self.max_jobs_merge is None else self.max_jobs_merge
        dep = merge_task(max_jobs=max_jobs_merge, tmp_folder=self.tmp_folder, config_dir=self.config_dir,
                         input_path=self.output_path, input_key=tmp_key, output_path=self.output_path,
                         output_key=self.output_key, number_of_labels=self._number_of_labels(),
                         prefix=self.prefix, dependency=dep)
        return dep

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'block_morphology': block_tasks.BlockMorphologyLocal.default_task_config(),
                        'merge_morphology': merge_tasks.MergeMorphologyLocal.default_task_config()})
        return configs
