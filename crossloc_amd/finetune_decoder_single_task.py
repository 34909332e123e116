"""Decoder fine-tuning entry point with the reference's options (finetune_decoder_single_task.py:29-136): a network of
`len(--encoders)` (or one fewer) frozen encoders loaded from the pretraining checkpoints, its decoder initialised from
the coord checkpoint's, on the MI355X path:

    python -m crossloc_amd.finetune_decoder_single_task urbanscape --task coord --encoders coord depth normal \
        --coord_weight <coord model.net> --depth_weight ... --normal_weight ... --semantics_weight ... --scene_dir ...

Data parallel under torch.distributed.run like crossloc_amd.train_single_task; see crossloc_amd/training.py.
"""
import logging
import os

from . import training


def _config_parser(argv=None):
    p = training.common_parser('Initialize a scene coordinate regression network.', sim_data_chunk_default=0.0)
    p.add_argument('--encoders', type=str, nargs='+', required=True)
    p.add_argument('--coord_weight', required=True)
    p.add_argument('--depth_weight', required=True)
    p.add_argument('--normal_weight', required=True)
    p.add_argument('--semantics_weight', required=True)
    p.add_argument('--reuse_coord_encoder', default=False, action="store_true")
    p.add_argument('--unfreeze_coord_encoder', default=False, action="store_true")
    return training.finish_options(p.parse_args(argv))


def check_encoders(encoders, coord_weight, depth_weight, normal_weight, semantics_weight):
    """utils/io.py:259-287: checkpoint paths of the listed encoders, the coord network's first."""
    for entry in encoders:
        assert entry in ['coord', 'depth', 'normal', 'semantics'], "encoder model {:s} is not supported!".format(entry)
    if 'coord' not in encoders:
        raise Exception("A coordinate regression network weight must be provided for decoder initialization!")
    weights = dict(coord=coord_weight, depth=depth_weight, normal=normal_weight, semantics=semantics_weight)
    paths = []
    for entry in sorted(set(encoders)):
        if not os.path.exists(weights[entry]):
            raise FileNotFoundError("--%s_weight %s does not exist" % (entry, weights[entry]))
        if entry == 'coord':
            paths.insert(0, weights[entry])
        else:
            paths.append(weights[entry])
    logging.info("{:d} network weights are to be loaded for reuse".format(len(paths)))
    return paths


def get_output_path(opt):
    """finetune_decoder_single_task.py:158-219 (the folder name; it lives under ./output)"""
    b = opt.scene + '-{:s}'.format(opt.task) + '-decoder_' + '_'.join(opt.encoders)
    if opt.reuse_coord_encoder:
        b = b.replace('_coord_', '_coord_free_' if opt.unfreeze_coord_encoder else '_coord_frozen_')
    else:
        b = b.replace('_coord_', '_')
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
    else:
        assert opt.sim_data_chunk == 0.0, "LHS sim data is disabled when pairwise sim-to-real data is used"
    b += training.data_suffix(opt, '-pairwise', '-zero_shot' if '-ft0.00' in opt.session else '-sim_only')
    if opt.tiny:
        b += '-tiny'
    if opt.network_in is not None and not (opt.auto_resume or opt.epoch_plus):
        b += '-resume'
    if opt.debug:
        b += '-DEBUG'
    return b


def main(argv=None):
    opt = _config_parser(argv)
    encoders_in = check_encoders(opt.encoders, opt.coord_weight, opt.depth_weight, opt.normal_weight,
                                 opt.semantics_weight)
    return training.run(opt, get_output_path(opt), encoders_in)


if __name__ == '__main__':
    main()
