"""Writes tests/golden/reference_configs.json: what ``boxinstseg_amd.load_config`` makes of every BoxInst config of the
reference (``configs/boxinst/*.py``) -- the mask-head dict, ``dist_params`` and ``data.samples_per_gpu`` -- so that the
test-suite checks the head built from them without the reference tree.

    python tests/golden/make_config_golden.py <reference checkout>
"""
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def extract(cfg_dir):
    import boxinstseg_amd as bx
    out = {}
    for path in sorted(glob.glob(os.path.join(cfg_dir, '*.py'))):
        cfg = bx.load_config(path)
        out[os.path.basename(path)] = dict(mask_head=cfg['model']['mask_head'], dist_params=cfg.get('dist_params'),
                                           samples_per_gpu=cfg['data']['samples_per_gpu'])
    return out


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    got = extract(os.path.join(sys.argv[1], 'configs', 'boxinst'))
    with open(os.path.join(HERE, 'reference_configs.json'), 'w') as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'{len(got)} configs')
