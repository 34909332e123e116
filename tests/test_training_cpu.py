"""CPU: the training drivers' host side - network configuration against the reference's config_network (names recorded by
tests/golden/make_training_configs.py), encoder checkpoint loading, option parsing, the data-parallel sampler and the
data sections."""
import json
import os

import pytest
import torch

from crossloc_amd import finetune_decoder_single_task as ft
from crossloc_amd import train_single_task as ts
from crossloc_amd import training

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "training_configs.json")) as f:
    CASES = json.load(f)


def _checkpoint(tmp_path, task, tiny, seed):
    torch.manual_seed(seed)
    c = training.TASK_CHANNELS[task]
    net = training.config_network(task, tiny, False, None if task == 'semantics' else 'MLE', task == 'semantics',
                                  torch.zeros(c))
    path = tmp_path / task / "model.net"
    path.parent.mkdir(parents=True, exist_ok=True)
    torch.save(training.state_dict(net), path)
    return str(path), net.state_dict()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_config_network_matches_the_reference(tmp_path, case):
    encoders_in = None
    if case["encoders"]:
        encoders_in = [_checkpoint(tmp_path, e, case["tiny"], i)[0] for i, e in enumerate(case["encoders"])]
    net = training.config_network(case["task"], case["tiny"], False, case["uncertainty"], case["fullsize"],
                                  torch.zeros(training.TASK_CHANNELS[case["task"]]), encoders_in, case["reuse"],
                                  case["unfreeze"])
    assert sorted(net.state_dict().keys()) == case["keys"]
    assert sorted(n for n, p in net.named_parameters() if p.requires_grad) == case["trainable"]


def test_finetune_network_is_initialised_from_the_checkpoints(tmp_path):
    paths, sds = zip(*[_checkpoint(tmp_path, e, False, i) for i, e in enumerate(("coord", "depth", "normal"))])
    net = training.config_network("coord", False, False, "MLE", False, torch.zeros(3), list(paths), True, False)
    sd = net.state_dict()
    for k, v in sds[0].items():
        if k.startswith("decoder."):
            assert torch.equal(sd[k], v), k
    for i, ref in enumerate(sds):                   # reuse_coord_encoder: encoders 1..3 are coord, depth, normal
        for k, v in ref.items():
            if k.startswith("encoder."):
                assert torch.equal(sd["mlr_encoder_%d.%s" % (i + 1, k[len("encoder."):])], v), (i, k)


def test_encoder_checkpoints_with_and_without_prefix_load_the_same_tensors(tmp_path):
    path, sd = _checkpoint(tmp_path, "depth", False, 3)
    bare = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    nets = []
    for weights in (sd, bare):
        torch.manual_seed(11)
        net = training.config_network("coord", False, False, "MLE", False, torch.zeros(3))
        training.load_module(net.encoder, weights, prefix="encoder.")
        nets.append(net.encoder.state_dict())
    assert nets[0].keys() == nets[1].keys()
    assert all(torch.equal(nets[0][k], nets[1][k]) and torch.equal(nets[0][k], bare[k]) for k in nets[0])
    with pytest.raises(KeyError):
        training.load_module(net.encoder, {k: v for k, v in bare.items() if k != "conv1.weight"})


def test_label_means_and_unknown_scenes():
    assert torch.equal(training.get_label_mean("urbanscape", "coord"), torch.tensor([-29.34, 184.17, 91.96]))
    assert torch.equal(training.get_label_mean("naturescape", "depth"), torch.tensor([241.47]))
    assert training.get_label_mean("urbanscape", "normal").shape == (2,)
    assert torch.equal(training.get_label_mean("naturescape", "semantics"), torch.zeros(6))
    with pytest.raises(NotImplementedError):
        training.get_label_mean("cambridge", "coord")
    with pytest.raises(NotImplementedError):
        training.get_nodata_value("cambridge")
    with pytest.raises(NotImplementedError):
        training.config_network("semantics", False, False, "MLE", True, torch.zeros(6))
    with pytest.raises(NotImplementedError):
        training.config_network("semantics", False, False, None, False, torch.zeros(6))


# the option sets of the python command lines in the reference's script_clean_training/*.sh (values substituted)
TRAIN_LINES = [
    "urbanscape --task coord --learningrate 1e-4 --epochs 1000 --batch_size 8 --inittolerance 50.0 --softclamp 100 "
    "--hardclamp 1000 --real_data_domain in_place --real_data_chunk 0.0 --sim_data_chunk 1.0 --uncertainty MLE "
    "--auto_resume --ckpt_dir ckpt --no_lr_scheduling --session clean_training",
    "urbanscape --task depth --fullsize --learningrate 1e-4 --epochs 1000 --batch_size 8 --softclamp 100 --hardclamp 10 "
    "--real_data_domain out_of_place --real_data_chunk 1.0 --sim_data_chunk 0.0 --uncertainty MLE --auto_resume --tiny "
    "--ckpt_dir ckpt --network_in a/model.net --session clean_training_x --no_lr_scheduling",
    "naturescape --task semantics --fullsize --real_data_chunk 1.0 --sim_data_chunk 0.0 --uncertainty none "
    "--no_lr_scheduling --real_only --session clean_training",
]
FINETUNE_LINES = [
    "urbanscape --task coord --coord_weight c --depth_weight d --normal_weight n --semantics_weight s "
    "--encoders coord depth normal --session x --learningrate 1e-4 --epochs 1000 --inittolerance 50.0 --batch_size 8 "
    "--softclamp 100 --hardclamp 1000 --real_data_domain in_place --real_data_chunk 1.0 --sim_data_chunk 0.0 "
    "--uncertainty MLE --auto_resume --ckpt_dir ckpt --reuse_coord_encoder --unfreeze_coord_encoder --no_lr_scheduling",
    "urbanscape --task coord --coord_weight c --depth_weight d --normal_weight n --semantics_weight s "
    "--encoders coord depth normal semantics --session x --real_data_chunk 1.0 --sim_data_chunk 0.0 --uncertainty MLE "
    "--tiny --reuse_coord_encoder --unfreeze_coord_encoder --no_lr_scheduling --real_only",
    "urbanscape --task coord --coord_weight c --depth_weight d --normal_weight n --semantics_weight s "
    "--encoders coord depth normal --real_data_chunk 0.0 --sim_data_chunk 1.0 --network_in a/model.net",
]


@pytest.mark.parametrize("line", TRAIN_LINES)
def test_train_parser_accepts_the_reference_options(line):
    opt = ts._config_parser(line.split() + ["--scene_dir", "d", "--max_steps", "3"])
    assert opt.uncertainty in (None, "MLE") and opt.max_steps == 3 and opt.scene_dir == "d"
    assert ts.get_output_path(opt).startswith(opt.scene + "-" + opt.task)


@pytest.mark.parametrize("line", FINETUNE_LINES)
def test_finetune_parser_accepts_the_reference_options(line):
    opt = ft._config_parser(line.split())
    assert opt.encoders[0] == "coord" and opt.uncertainty in (None, "MLE")
    assert "-decoder_" in ft.get_output_path(opt)


def test_parser_defaults_follow_the_reference():
    opt = ts._config_parser(["urbanscape", "--task", "coord"])
    assert (opt.batch_size, opt.epochs, opt.learningrate, opt.sim_data_chunk, opt.real_data_chunk) == (4, 50, 2e-4, 1.0, 1.0)
    assert (opt.inittolerance, opt.mindepth, opt.softclamp, opt.hardclamp, opt.uncertainty) == (50.0, 0.1, 100, 1000, None)
    f = ft._config_parser("urbanscape --task coord --encoders coord --coord_weight c --depth_weight d --normal_weight n "
                          "--semantics_weight s".split())
    assert f.sim_data_chunk == 0.0 and not f.reuse_coord_encoder and not f.unfreeze_coord_encoder


def test_check_encoders_puts_coord_first(tmp_path):
    paths = {}
    for e in ("coord", "depth", "normal", "semantics"):
        paths[e] = str(tmp_path / e)
        open(paths[e], "w").close()
    got = ft.check_encoders(["normal", "depth", "coord"], paths["coord"], paths["depth"], paths["normal"], paths["semantics"])
    assert got == [paths["coord"], paths["depth"], paths["normal"]]
    with pytest.raises(Exception):
        ft.check_encoders(["depth"], paths["coord"], paths["depth"], paths["normal"], paths["semantics"])


@pytest.mark.parametrize("n,world,batch", [(10, 1, 4), (10, 2, 2), (13, 4, 3), (8, 8, 1)])
def test_sampler_shards_are_disjoint_and_seeded(n, world, batch):
    for epoch in range(3):
        shards = [training.epoch_batches(n, epoch, batch, r, world) for r in range(world)]
        assert len({len(s) for s in shards}) == 1                       # every rank runs the same number of steps
        flat = [i for s in shards for b in s for i in b]
        assert len(flat) == len(set(flat)) == n // world * world
        assert all(len(b) <= batch for s in shards for b in s)
        assert shards == [training.epoch_batches(n, epoch, batch, r, world) for r in range(world)]
    assert training.epoch_batches(n, 0, n, 0, 1) != training.epoch_batches(n, 1, n, 0, 1) or n < 3


def test_training_sections_follow_the_reference(tmp_path):
    for d in ("train_sim", "train_drone_real", "train_drone_sim", "train_oop_drone_real_chunk_0.50"):
        (tmp_path / d).mkdir()
    assert training.get_training_dirs(str(tmp_path), "in_place", 1.0, 1.0, False) == [
        str(tmp_path / d) for d in ("train_sim", "train_drone_real", "train_drone_sim")]
    assert training.get_training_dirs(str(tmp_path), "out_of_place", 0.5, 0.0, True) == [
        str(tmp_path / "train_oop_drone_real_chunk_0.50")]
    with pytest.raises(FileNotFoundError, match="train_sim_chunk_0.25"):
        training.get_training_dirs(str(tmp_path), "in_place", 0.0, 0.25, False)


def test_auto_resume_starts_fresh_then_continues_from_the_output_folder(tmp_path):
    out, other = tmp_path / "out", tmp_path / "pretrained"
    out.mkdir(); other.mkdir()
    torch.save({}, other / "resume.pt")
    line = "urbanscape --task coord --uncertainty MLE --auto_resume --network_in %s" % (other / "model.net")
    opt = ts._config_parser(line.split())
    assert training.resume_source(opt, str(out)) is None               # first run: fresh, --network_in initialises
    torch.save({}, out / "resume.pt")
    assert training.resume_source(opt, str(out)) == str(out / "resume.pt")   # never the --network_in folder's state
    plus = ts._config_parser(("urbanscape --task coord --epoch_plus --network_in %s" % (other / "model.net")).split())
    assert training.resume_source(plus, str(out)) == str(other / "resume.pt")
    with pytest.raises(ValueError):
        training.resume_source(ts._config_parser("urbanscape --task coord --epoch_plus".split()), str(out))
