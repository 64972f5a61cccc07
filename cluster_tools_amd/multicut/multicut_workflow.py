"""MulticutWorkflow (reference: cluster_tools/multicut/multicut_workflow.py:45-67): the same
parameters (problem_path / n_scales / assignment_path / assignment_key) and get_config.  The
reference solves hierarchically: n_scales rounds of SolveSubproblems and ReduceProblem on the
per-block sub-graphs, then SolveGlobal on the reduced problem.  Here the graph is computed whole
and there are no sub-graphs, so the workflow is the SolveGlobal task on the whole problem:
n_scales must be 0, anything else raises NotImplementedError.  target must be 'local'."""
from cluster_tools_amd.luigi_compat import Parameter, IntParameter
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.multicut import solve_global as solve_tasks


class MulticutWorkflow(WorkflowBase):
    problem_path = Parameter()
    n_scales = IntParameter()
    assignment_path = Parameter()
    assignment_key = Parameter()

    def requires(self):
        if self.n_scales != 0:
            raise NotImplementedError('n_scales %s: the multicut is solved on the whole graph in one device call, '
                                      'there are no sub-problems to solve hierarchically; n_scales must be 0'
                                      % str(self.n_scales))
        solve_task = getattr(solve_tasks, self._get_task_name('SolveGlobal'))
        return solve_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                          problem_path=self.problem_path, assignment_path=self.assignment_path,
                          assignment_key=self.assignment_key, scale=self.n_scales, dependency=self.dependency)

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'solve_global': solve_tasks.SolveGlobalLocal.default_task_config()})
        return configs
