"""Generates training_configs.json by importing the REFERENCE Python (utils/learning.py:266-398 config_network) with stub
modules for the packages it imports but this path never uses.  Run with
`python3 -B tests/golden/make_training_configs.py <CrossLoc checkout>` so no bytecode is written into the reference tree.

For every network configuration the CrossLoc scripts train (script_clean_training/*.sh: encoder pretraining of coord /
depth / normal with MLE uncertainty and of full-size semantics without, tiny on and off; decoder fine-tuning of the coord
task with --encoders coord depth normal [semantics], with and without --reuse_coord_encoder / --unfreeze_coord_encoder)
the fixture stores the state_dict keys and the names of the trainable parameters - names only, no weights.
"""
import json
import os
import sys
import tempfile
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
for n in ['git', 'cv2', 'transforms3d', 'transforms3d.quaternions', 'skimage', 'skimage.io', 'skimage.color',
          'skimage.transform', 'torchvision', 'torchvision.transforms', 'dsacstar']:
    sys.modules[n] = types.ModuleType(n)
q = sys.modules['transforms3d.quaternions']; q.mat2quat = q.quat2mat = None
t = sys.modules['skimage.transform']; t.rotate = t.resize = None
sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
sys.path.insert(0, os.path.abspath(sys.argv[1]))
from networks.networks import TransPoseNet                      # noqa: E402
from utils.learning import config_network                       # noqa: E402

CHANNELS = {'coord': 3, 'depth': 1, 'normal': 2, 'semantics': 6}


def pretrain_cases():
    for task in ('coord', 'depth', 'normal', 'semantics'):
        for tiny in (False, True):
            unc = None if task == 'semantics' else 'MLE'
            yield dict(name="train-%s%s" % (task, "-tiny" if tiny else ""), task=task, tiny=tiny, uncertainty=unc,
                       fullsize=task == 'semantics', encoders=None, reuse=False, unfreeze=False)


def finetune_cases():
    for encs in (('coord', 'depth', 'normal'), ('coord', 'depth', 'normal', 'semantics')):
        for reuse, unfreeze in ((False, False), (True, False), (True, True)):
            for tiny in (False, True):
                yield dict(name="finetune-%s%s%s%s" % ("_".join(encs), "-reuse" if reuse else "",
                                                       "-unfreeze" if unfreeze else "", "-tiny" if tiny else ""),
                           task='coord', tiny=tiny, uncertainty='MLE', fullsize=False, encoders=list(encs),
                           reuse=reuse, unfreeze=unfreeze)


def main():
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for case in list(pretrain_cases()) + list(finetune_cases()):
            encoders_in = None
            if case['encoders']:
                encoders_in = []
                for e in case['encoders']:
                    net = TransPoseNet(torch.zeros(CHANNELS[e]), case['tiny'], False, 2, 2, CHANNELS[e],
                                       0 if e == 'semantics' else 1, full_size_output=e == 'semantics')
                    path = os.path.join(tmp, e, 'model.net')
                    os.makedirs(os.path.dirname(path), exist_ok=True)
                    torch.save(net.state_dict(), path)
                    encoders_in.append(path)
            mean = torch.zeros(CHANNELS[case['task']])
            network, _, _, _ = config_network('urbanscape', case['task'], case['tiny'], False, case['uncertainty'],
                                              case['fullsize'], mean, 1e-4, True, False, False, None, tmp,
                                              encoders_in, case['reuse'], case['unfreeze'])
            out.append(dict(case, keys=sorted(network.state_dict().keys()),
                            trainable=sorted(n for n, p in network.named_parameters() if p.requires_grad)))
    with open(os.path.join(HERE, 'training_configs.json'), 'w') as f:
        json.dump(out, f, indent=0)


if __name__ == '__main__':
    main()
