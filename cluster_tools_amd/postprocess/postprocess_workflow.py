"""SizeFilterWorkflow (reference: cluster_tools/postprocess/postprocess_workflow.py:24-110): the
same parameters and task chain FindUniques(return_counts) -> SizeFilterBlocks ->
BackgroundSizeFilter, with the reference's tmp artefacts and logs.  relabel=True: the reference
chains a RelabelWorkflow (three more passes over the volume) behind the filter; here the
BackgroundSizeFilter job filters and relabels in one device call and writes the
`relabel_size_filter` assignment table and the new `maxId` itself.  hmap_path != '' (the
reference's FillingSizeFilter, a watershed fill) is not available.  target must be 'local'."""
from cluster_tools_amd.luigi_compat import Parameter, IntParameter, BoolParameter
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.relabel import find_uniques as unique_tasks
from cluster_tools_amd.postprocess import size_filter_blocks as size_filter_tasks
from cluster_tools_amd.postprocess import background_size_filter as bg_tasks


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
