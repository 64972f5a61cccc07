"""stdout logging contract of the job scripts (cluster_tools/utils/function_utils.py:7-16):
LocalTask.check_jobs reads the last line of each job log and expects 'processed job <i>'.
Plus what every job script starts and ends with (job_config, run_job).  No numpy / torch import
here: the fused job is torch-free and a one-shot job's start time counts."""
import json
import os
import sys
from datetime import datetime


def log(msg):
    print('%s: %s' % (str(datetime.now()), msg), flush=True)


def log_block_success(block_id):
    print('%s: processed block %i' % (str(datetime.now()), block_id), flush=True)


def log_blocks_success(block_list):
    for block_id in block_list:
        log_block_success(block_id)


def log_job_success(job_id):
    print('%s: processed job %i' % (str(datetime.now()), job_id), flush=True)


def job_config(job_id, config_path):
    """The job prologue: its two log lines, then the job's config."""
    log('start processing job %i' % job_id)
    log('reading config from %s' % config_path)
    with open(config_path) as f:
        return json.load(f)


def run_job(fn):
    """`if __name__ == '__main__'` of a job script run as `<script> <tmp>/<task>_job[_<prefix>]_<id>.config`:
    fn(job_id, config_path)."""
    path = sys.argv[1]
    assert os.path.exists(path), path
    job_id = int(os.path.split(path)[1].split('.')[0].split('_')[-1])
    fn(job_id, path)
