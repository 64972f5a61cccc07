"""What the watershed tasks (distance_transform.py, seeds.py, watershed_from_seeds.py) share: the
task with the reference's surface (watershed.py:43-48, :74-75) and the job's channel read."""
import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, TaskParameter
from cluster_tools_amd.cluster_tasks import DummyTask
import cluster_tools_amd.utils.volume_utils as vu


class WatershedTaskBase(Task):
    """One GPU job over the blocks of the input; a subclass sets task_name, src_file, output_dtype
    and its default_task_config, and may override check_config and extra_paths."""
    input_path = Parameter()
    input_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    mask_path = Parameter(default='')
    mask_key = Parameter(default='')
    dependency = TaskParameter(default=DummyTask())

    output_dtype = 'uint64'

    def check_config(self, config, shape, block_shape):
        pass

    def extra_paths(self):
        return {}

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        shape = vu.get_shape(self.input_path, self.input_key)
        if len(shape) == 4:                           # channels first (watershed.py:74-75)
            shape = shape[1:]
        config = self.get_task_config()
        assert config.get('agglomerate_channels', 'mean') in ('mean', 'max', 'min')
        self.check_config(config, shape, block_shape)
        chunks = tuple(bs // 2 for bs in block_shape)
        chunks = tuple(max(1, min(ch, sh)) for ch, sh in zip(chunks, shape))
        with vu.file_reader(self.output_path) as f:
            f.require_dataset(self.output_key, shape=shape, chunks=chunks, compression='gzip',
                              dtype=self.output_dtype)
        config.update({'input_path': self.input_path, 'input_key': self.input_key, **self.extra_paths(),
                       'output_path': self.output_path, 'output_key': self.output_key,
                       'block_shape': block_shape})
        if self.mask_path != '':
            assert self.mask_key != ''
            config.update({'mask_path': self.mask_path, 'mask_key': self.mask_key})
        block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        self._write_log('scheduling %i blocks to be processed' % len(block_list))
        self.run_jobs(1, block_list, config)          # one GPU job for the whole volume


def check_dt_config(config, task):
    """The distance-transform keys this path does not support, for the task and its job."""
    if any(int(h) != 0 for h in (config.get('halo') or [0, 0, 0])):
        raise NotImplementedError('a non-zero halo is not supported by the %s task' % task)
    if config.get('apply_dt_2d', True) and config.get('pixel_pitch') is not None:
        raise ValueError('pixel_pitch needs apply_dt_2d = False (watershed.py:152)')


def read_channels(config, shape, box=None):
    """The job's float32 input (normalize's astype('float32')) over `box` of the volume (whole when
    None); shape is the input dataset's.  4-D input: the channels channel_begin:channel_end of it
    (_read_data, watershed.py:268-277, watershed_from_seeds.py:127-139)."""
    from cluster_tools_amd.thresholded_components.block_components import _read
    box = list(box or [(0, s) for s in shape[-3:]])
    if len(shape) == 4:
        c0, c1, _ = slice(config.get('channel_begin', 0), config.get('channel_end', None)).indices(shape[0])
        if c1 <= c0:
            raise ValueError('empty channel range %s:%s' % (config.get('channel_begin', 0), config.get('channel_end')))
        box = [(c0, c1)] + box
    return _read(config['input_path'], config['input_key'], box=box, dtype=np.float32)
