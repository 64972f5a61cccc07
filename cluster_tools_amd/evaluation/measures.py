#! /usr/bin/python
"""Measures task + job (reference: cluster_tools/evaluation/measures.py).

Same task surface as the reference MeasuresBase (measures.py:23-56: task_name 'measures', one
job, output_path JSON with 'vi-split', 'vi-merge', 'adapted-rand-error', 'rand-index').  The
reference reads the overlaps NodeLabelWorkflow serialized (node_labels/block_node_labels.py:
133-166 + merge_node_labels.py); here the one GPU job reads the segmentation and ground truth
and cc_evaluate computes the same overlaps (block grid of the global config, ws.sum() == 0 block
skip, gt ignore label) and the contingency-table measures on the MI355X in one pass
(cluster_tools_amd/csrc/cc_eval.hip).  Parameters are therefore seg / gt datasets instead of
input_path / overlap_key.
"""
import json
import os

from cluster_tools_amd.luigi_compat import Task, Parameter, TaskParameter, BoolParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context, read_labels_u64, labels_to_device


class MeasuresBase(Task):
    task_name = 'measures'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    seg_path = Parameter()
    seg_key = Parameter()
    gt_path = Parameter()
    gt_key = Parameter()
    output_path = Parameter()
    ignore_label = BoolParameter(default=True)
    dependency = TaskParameter(default=DummyTask())

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        config = self.get_task_config()
        shape = vu.get_shape(self.seg_path, self.seg_key)
        assert tuple(shape) == tuple(vu.get_shape(self.gt_path, self.gt_key)), 'seg / gt shapes differ'
        assert len(shape) == 3, str(len(shape))
        config.update({'seg_path': self.seg_path, 'seg_key': self.seg_key, 'gt_path': self.gt_path,
                       'gt_key': self.gt_key, 'output_path': self.output_path,
                       'ignore_label': 0 if self.ignore_label else None, 'block_shape': block_shape})
        self.run_jobs(1, None, config)


class MeasuresLocal(MeasuresBase, LocalTask):
    pass


def measures(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    seg = read_labels_u64(config['seg_path'], config['seg_key'])
    gt = read_labels_u64(config['gt_path'], config['gt_key'])
    with job_context() as (ctx, dev):
        r = ctx.evaluate(labels_to_device(seg, dev), labels_to_device(gt, dev),
                         config['block_shape'], ignore_label=config['ignore_label'])
    fu.log('contingency table: %i pairs over %i points' % (r['n_pairs'], r['n_points']))
    results = {'vi-split': r['vi_split'], 'vi-merge': r['vi_merge'],
               'adapted-rand-error': r['adapted_rand_error'], 'rand-index': r['rand_index']}
    with open(config['output_path'], 'w') as f:
        json.dump(results, f)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(measures)
