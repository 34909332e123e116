"""End-to-end DSAC* training of an initialised scene coordinate network: the expected pose loss of the differentiable solver,
through the network, on the MI355X path:

    python -m crossloc_amd.train_e2e urbanscape --network_in model.net --scene_dir <dataset folder> ...
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m crossloc_amd.train_e2e ...

The options of training.common_parser (data sections, --tiny, --uncertainty, --auto_resume, --max_steps, ...) plus the
solver's.  Their defaults follow DSAC*'s published train_e2e.py; the CrossLoc reference has no such script, so they are
defaults, not parity claims.  --network_in is required: the expected pose loss only has a useful gradient around an
initialised network.  --init_weight w > 0 keeps the coord loss in the step, w * coord gradient + pose gradient.

Augmentation: colour jitter and the per-batch scale stay; rotation is OFF - the batched augmentation does not rotate the
ground-truth poses (as the reference's, data.batch_resize), and a pose loss on rotated frames would be wrong.  --mode rgbd
reads the depth labels, takes --threshold and --maxpixelerror in centimetres, and fixes the scale to 1: the RGB-D kernels
take at most dsacstar.RGBD_MAX_CELLS cells (60 x 90 fits, 90 x 135 does not).

See crossloc_amd/training.py (make_e2e_step, Trainer) and loss.expected_pose_loss_and_output_gradient.
"""
from . import training
from .dsacstar import RANSAC_SEED


def _parser():
    p = training.common_parser('Train a scene coordinate regression network end to end.', sim_data_chunk_default=1.0,
                               task='coord')
    p.set_defaults(learningrate=1e-6)
    p.add_argument('--mode', type=str, default='rgb', choices=('rgb', 'rgbd'),
                   help='rgb: PnP hypotheses; rgbd: Kabsch hypotheses from the depth labels')
    p.add_argument('--hypotheses', type=int, default=64, help='hypotheses per frame')
    p.add_argument('--threshold', type=float, default=10, help='inlier threshold (rgb: pixels, rgbd: centimetres)')
    p.add_argument('--inlieralpha', type=float, default=100, help='softness of the inlier count')
    p.add_argument('--maxpixelerror', type=float, default=100,
                   help='clamp of a residual (rgb: pixels, rgbd: centimetres)')
    p.add_argument('--weightrot', type=float, default=1.0, help='weight of the rotation part of the pose loss')
    p.add_argument('--weighttrans', type=float, default=100.0, help='weight of the translation part of the pose loss')
    p.add_argument('--clip_norm', type=float, default=0.0,
                   help='clip the pose gradient of a frame to this norm (0: no clipping)')
    p.add_argument('--init_weight', type=float, default=0.0,
                   help='weight of the coord loss kept in the step (0: the pose loss alone)')
    p.add_argument('--seed', type=int, default=RANSAC_SEED, help="the sampler's seed; step k draws with seed + k")
    return p


def _config_parser(argv=None):
    p = _parser()
    opt = training.finish_options(p.parse_args(argv))
    if opt.task != 'coord':
        p.error("end-to-end training is for the coord task")
    if opt.network_in is None:
        p.error("--network_in is required: end-to-end training starts from an initialised network")
    if opt.fullsize:
        p.error("--fullsize: the solver works on the 8x subsampled grid")
    if opt.real_only:
        assert opt.sim_data_chunk == 0
    return opt


def dataset_options(opt):
    """What the end-to-end step needs of CamLocDataset: no rotation; --mode rgbd: the depth labels and the scale fixed to 1."""
    kw = dict(coord=True, depth=opt.mode == 'rgbd', aug_rotation=0)
    if opt.mode == 'rgbd':
        kw.update(aug_scale_min=1, aug_scale_max=1)
    return kw


def get_output_path(opt):
    """The folder name under ./output, in the manner of train_single_task.get_output_path."""
    b = opt.scene + '-e2e-' + opt.mode
    if opt.session != '':
        b += '-s' + opt.session
    if opt.grayscale:
        b += '-gray'
    b += '-no_unc' if opt.uncertainty is None else '-unc-{:s}'.format(opt.uncertainty)
    b += '-e{:d}-lr{:.8f}'.format(opt.epochs, opt.learningrate)
    b += training.data_suffix(opt, '-pairs')
    if opt.tiny:
        b += '-tiny'
    if opt.debug:
        b += '-DEBUG'
    return b


def main(argv=None):
    opt = _config_parser(argv)
    return training.run(opt, get_output_path(opt), e2e=True, dataset_options=dataset_options(opt))


if __name__ == '__main__':
    main()
