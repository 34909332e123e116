"""End-to-end DSAC* training of an initialised scene coordinate network: the expected pose loss of the differentiable solver,
through the network, on the MI355X path:

    python -m crossloc_amd.train_e2e urbanscape --network_in model.net --scene_dir <dataset folder> ...
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m crossloc_amd.train_e2e ...

The options of training.common_parser (data sections, --tiny, --uncertainty, --auto_resume, --max_steps, ...) plus the
solver's.  Their defaults follow DSAC*'s published train_e2e.py; the CrossLoc reference has no such script, so they are
defaults, not parity claims.  --network_in is required: the expected pose loss only has a useful gradient around an
initialised network.  --init_weight w > 0 keeps the coord loss in the step, w * coord gradient + pose gradient.

Augmentation: colour jitter and the per-batch scale always; in-plane rotation with --aug_rotation DEG (default 0: none;
DSAC*'s own recipe trains with 30).  Each frame of a mini-batch then draws its own angle in +-DEG, frame and label maps are
rotated by it, and the ground-truth pose becomes P * Rz(angle) (CamLocDataset(rotate_poses=True), data.batch_resize_posed),
so the pose loss sees the pose of the frame it is given.  The reference's batched augmentation, and this package's default,
rotate the frames of a mini-batch by one common angle and leave the poses alone - no input for a pose loss, which is why
the default here is no rotation.  --mode rgbd reads the depth labels, takes --threshold and --maxpixelerror in
centimetres, and fixes the scale to 1: the RGB-D kernels take at most dsacstar.RGBD_MAX_CELLS cells (60 x 90 fits, 90 x 135
does not); its depth label rotates like any label map (fill -1: nothing measured), the depth along the optical axis being
what an in-plane rotation leaves unchanged.  --aug_canvas: fixed-size augmentation (CamLocDataset(canvas=True),
data.batch_canvas) - every frame draws its own scale and, with --aug_rotation DEG, its own angle (at 0: scale only), and is
warped onto a canvas of its own size; the solver and the --init_weight coord term read one focal length per frame.  The
label grid stays 60 x 90, so --mode rgbd keeps the scale range 2/3 - 3/2 with it.  --mask labels (--mode rgb): the cells whose
coord label is the scene's nodata value - sky, water, the empty border --aug_canvas and --aug_rotation leave around a warped
frame - are masked out of the solver's backward pass, as --mode rgbd drops depth holes by itself.  --mask_sampler compact (with
--mask labels): the solver draws the cells of a try from the usable cells only; under the default, reject, the expected tries
of a hypothesis grow as (usable fraction)^-4 and a frame that keeps a tenth of its cells exhausts every hypothesis.

See crossloc_amd/training.py (make_e2e_step, Trainer) and loss.expected_pose_loss_and_output_gradient.
"""
from . import training
from .dsacstar import MASK_SAMPLERS, RANSAC_SEED


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
    p.add_argument('--aug_rotation', type=float, default=0.0, metavar='DEG',
                   help='rotate each frame by its own angle in +-DEG, and its ground-truth pose with it (0: no rotation)')
    p.add_argument('--mask', type=str, default='none', choices=('none', 'labels'),
                   help='labels: cells whose coord label is nodata (sky, water, the empty border of a warped frame) are no '
                        'evidence for the solver and get no pose gradient (--mode rgb)')
    p.add_argument('--mask_sampler', type=str, default='reject', choices=MASK_SAMPLERS,
                   help='how the masked solver draws the cells of a try (with --mask labels); compact: from the usable cells '
                        'only, for masks that keep a minority of the cells')
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
    if opt.aug_rotation < 0:
        p.error("--aug_rotation is the half width of the angle range: it cannot be negative")
    if opt.mask == 'labels' and opt.mode == 'rgbd':
        p.error("--mask labels is for --mode rgb: the RGB-D solver drops depth holes itself and takes no mask")
    if opt.mask_sampler != 'reject' and opt.mask != 'labels':
        p.error("--mask_sampler %s is the masked solver's: it needs --mask labels" % opt.mask_sampler)
    if opt.real_only:
        assert opt.sim_data_chunk == 0
    return opt


def dataset_options(opt):
    """What the end-to-end step needs of CamLocDataset: no rotation, or with --aug_rotation one per frame with the poses
    rotated along; --mode rgbd: the depth labels and the scale fixed to 1.  --aug_canvas: a scale and an angle (in
    +-aug_rotation, 0: none) per frame at a fixed size, in either mode with the dataset's own scale range."""
    kw = dict(coord=True, depth=opt.mode == 'rgbd', aug_rotation=0)
    if opt.aug_canvas:
        kw.update(aug_rotation=opt.aug_rotation, canvas=True)
        return kw
    if opt.aug_rotation > 0:
        kw.update(aug_rotation=opt.aug_rotation, rotate_poses=True)
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
    if opt.aug_rotation > 0:
        b += '-rot{:g}'.format(opt.aug_rotation)
    if opt.aug_canvas:
        b += '-canvas'
    if opt.mask != 'none':
        b += '-mask' + opt.mask
    if getattr(opt, 'mask_sampler', 'reject') != 'reject':
        b += '-' + opt.mask_sampler
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
