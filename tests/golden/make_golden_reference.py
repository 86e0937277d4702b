"""Generate tests/golden/reference_layouts.json and tests/golden/reference_fresh.npz by running the REFERENCE
(build container only: oracle/ref_import.py locates the reference checkout and loads it in place, never copied).

    python tests/golden/make_golden_reference.py

They hold the reference's side of the CPU tests that compare the build with the reference module itself, so that
those tests run wherever the repository does:

  layouts  for six cases of cases.py: the state_dict key order and shapes of the reference module, its parameter count
  configs  for every shipped YAML: the NETWORK section and the DATASET fields that decide the number of views, as the
           reference's core/config.py resolves them (update_config), and the state_dict layout and num_views of the
           module the reference's get_multiview_mpl_net builds from that config
  fresh    reference outputs on other weights and inputs than the goldens' (detrng seeds 99 / 123, batch 6)

Fixtures are data only (names, shapes, config values, output arrays); no reference source.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from openmpl_amd import detrng            # noqa: E402
from oracle import ref_import             # noqa: E402
from tests.golden.cases import CASES        # noqa: E402

LAYOUTS = ["chosen_v4_b8_l2", "full_v4_b8_l2", "kadkhod_v3_b3_l2", "deep_head_v3_b3_l2", "conf_add_v3_b3_l2",
           "linear_wmean_v3_b3_l2"]
FRESH = ["chosen_v4_b8_l2", "full_v4_b8_l2", "conf_attnw_v3_b3_l2", "kadkhod_v3_b3_l2"]
FRESH_WSEED, FRESH_ISEED, FRESH_BATCH = 99, 123, 6
# the DATASET fields MultiView_MPL_G reads (the number of views)
VIEW_FIELDS = ["TEST_DATASET", "TRAIN_VIEWS", "USE_HELPER_CAMERAS", "TRAIN_VIEWS_HELPER", "TRAIN_ON_ALL_CAMERAS",
               "TEST_ON_ALL_CAMERAS", "N_VIEWS_TRAIN_TEST_ALL"]


def layout(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def plain(v):
    """Config values as JSON data (the reference keeps some of them as numpy arrays)."""
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    return v


def main():
    by_name = {c["name"]: c for c in CASES}
    layouts = {}
    for name in LAYOUTS:
        m = ref_import.build_reference(dict(by_name[name]["flags"], drop_path_rate=0.1))
        layouts[name] = dict(state_dict=layout(m), n_parameters=sum(p.numel() for p in m.parameters()))
    configs = []
    ref_mod = ref_import.load_reference_module()
    for y in ref_import.shipped_yamls():
        cfg = ref_import.load_reference_config(y)
        ref = ref_mod.get_multiview_mpl_net(cfg, is_train=False)
        configs.append(dict(yaml=os.path.relpath(y, ref_import.CONFIG_DIR), MODEL=cfg.MODEL,
                            DATASET={k: plain(cfg.DATASET[k]) for k in VIEW_FIELDS}, NETWORK=plain(cfg.NETWORK),
                            state_dict=layout(ref), num_views=ref.features.num_views))
    with open(os.path.join(HERE, "reference_layouts.json"), "w") as f:
        json.dump(dict(layouts=layouts, configs=configs, torch=torch.__version__), f, sort_keys=True, separators=(",", ":"))
        f.write("\n")

    rec = dict(meta=np.frombuffer(json.dumps(dict(wseed=FRESH_WSEED, iseed=FRESH_ISEED, batch=FRESH_BATCH,
                                                  torch=torch.__version__)).encode(), dtype=np.uint8))
    for name in FRESH:
        flags = by_name[name]["flags"]
        m = ref_import.build_reference(dict(flags, drop_path_rate=0.1))
        detrng.fill_module_(m, seed=FRESH_WSEED)
        p, r, c = detrng.make_inputs(FRESH_BATCH, flags["num_views"], seed=FRESH_ISEED)
        with torch.no_grad():
            out = m([torch.from_numpy(x.copy()) for x in p], rays=[torch.from_numpy(x) for x in r],
                    centers=[torch.from_numpy(x) for x in c])
        rec[name] = (out[0] if isinstance(out, tuple) else out).numpy()
        print("%-24s out|max|=%.4f" % (name, float(np.abs(rec[name]).max())))
    np.savez_compressed(os.path.join(HERE, "reference_fresh.npz"), **rec)


if __name__ == "__main__":
    main()
