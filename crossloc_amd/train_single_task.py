"""Encoder pretraining entry point with the reference's options (train_single_task.py:32-117), on the MI355X path:

    python -m crossloc_amd.train_single_task urbanscape --task coord --scene_dir <dataset folder> ...
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m crossloc_amd.train_single_task ...

See crossloc_amd/training.py for the step, the sampler, the checkpoints and resume.pt.
"""
from . import training


def _config_parser(argv=None):
    p = training.common_parser('Initialize a scene coordinate regression network.', sim_data_chunk_default=1.0)
    opt = training.finish_options(p.parse_args(argv))
    if opt.real_only:
        assert opt.sim_data_chunk == 0
    return opt


def get_output_path(opt):
    """train_single_task.py:129-175 (the folder name; it lives under ./output)"""
    b = opt.scene + '-{:s}'.format(opt.task)
    if opt.session != '':
        b += '-s' + opt.session
    if opt.grayscale:
        b += '-gray'
    b += '-no_unc' if opt.uncertainty is None else '-unc-{:s}'.format(opt.uncertainty)
    if opt.fullsize:
        b += '-fullsize'
    b += ('-e{:d}-lr{:.4f}' if opt.learningrate >= 1e-4 else '-e{:d}-lr{:.6f}').format(opt.epochs, opt.learningrate)
    if opt.real_data_chunk == 0.0:
        assert opt.sim_data_chunk > 0
    b += training.data_suffix(opt, '-pairs')
    if opt.tiny:
        b += '-tiny'
    if opt.network_in is not None and not (opt.auto_resume or opt.epoch_plus):
        b += '-finetune'
    if opt.debug:
        b += '-DEBUG'
    return b


def main(argv=None):
    opt = _config_parser(argv)
    return training.run(opt, get_output_path(opt))


if __name__ == '__main__':
    main()
