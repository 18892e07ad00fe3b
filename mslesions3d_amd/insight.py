"""Prior fit report — the quantitative version of the reference's ``lesions3d/model_insight.py:show_prior_boxes`` and
``stats_objects.py``: before any training, could the prior boxes match the lesions of this data set at all?

    python -m mslesions3d_amd.insight -d DATA -dn NAME -pl "3 5 7" -th 0.1 0.2 --size_bins 27,125,1000 -o OUT
    python -m mslesions3d_amd.insight -dm lesions -d RAW --centers C1 --spatial_size 96 96 96 --scale_factors 0.5,0.75,1,1.5,2 -o OUT

The priors are the ones ``train.py`` would build from ``-pl -sc -bpl -minos -maxos`` for the input the data flags give
(``--spatial_size``, or ``--patch_size`` with the tiles ``predict --views tiles`` shows the network); the matching is
``MultiBoxLoss``'s at ``-th``.  ``OUT/prior_fit.json`` holds ``utils.prior_fit_summary`` for them: per threshold and lesion
size bin the lesions that are matchable (best IoU >= threshold), positive only through the force-match, or orphaned (no
positive prior: they contribute nothing to either loss term), positives per lesion and per feature map, best-IoU quantiles,
and the box extents per axis.  ``--scale_factors`` adds one block per factor (all scales
multiplied by it; one ``msl_make_priors`` round and one ``msl_prior_fit`` call each, the ground truth uploaded once) and
names the factor with the fewest orphaned, then the most matchable lesions as ``"suggested"``.  ``--draw_priors 1`` writes the
priors of every feature map over the first case as ``sub-*_prior-boxes_fmap-F.npy`` (``utils.draw_boxes(style="edges")``).
"""
import argparse
import json
import os
from os.path import join as pjoin

import numpy as np
import torch

from .eval import BATCH, batch_voxels, float_list, size_bin_list
from .train import input_images_of, patch_options_of, segmentation_of

MAX_DRAWN_PRIORS = 32766  # utils.draw_boxes: int16 ids


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    # model_insight.py
    p.add_argument('-d', '--dataset_path', type=str, default=r'../data/artificial_dataset')
    p.add_argument('-dn', '--dataset_name', type=str, default=None)
    p.add_argument('-p', '--percentage', type=float, default=1.)
    # the prior-defining flags of train.py
    p.add_argument('-pl', '--prediction_layers', type=str, default="3 5 7")
    p.add_argument('-sc', '--scales', type=json.loads, default="{}")
    p.add_argument('-bpl', '--boxes_per_location', type=int, default=2)
    p.add_argument('-minos', '--min_object_size', type=int, default=6)
    p.add_argument('-maxos', '--max_object_size', type=int, default=14)
    p.add_argument('-th', '--threshold', type=float, default=[0.1, 0.2], nargs='+')
    # the data flags of eval.py
    p.add_argument('-dm', '--data_module', choices=["example", "lesions"], default="example")
    p.add_argument('--centers', type=str, nargs='+', default=['CHUV_RIM_OK', 'BASEL_INSIDER_OK'])
    p.add_argument('--spatial_size', type=int, nargs=3, default=[250, 300, 300], metavar=('D', 'H', 'W'))
    p.add_argument('-ii', '--input_images', type=str, nargs='+', default=["FLAIR"])
    p.add_argument('--segmentation', type=str, default="labeled_lesions", metavar='NAME',
                   help="as train.py: a mask name without 'labeled' in it is a binary mask")
    p.add_argument('-ps', '--predict_subset', type=str, choices=['train', 'validation', 'test', 'all'], default=r'train')
    p.add_argument('-nw', '--num_workers', type=int, default=0)
    p.add_argument('--patch_size', type=int, nargs=3, default=None, metavar=('D', 'H', 'W'))
    p.add_argument('--tile_margin', type=int, nargs=3, default=[8, 8, 8], metavar=('D', 'H', 'W'))
    p.add_argument('--size_bins', type=size_bin_list, default=None,
                   help="lesion size bins: comma-separated ascending bounding-box volumes in voxels, e.g. 27,125,1000")
    p.add_argument('--scale_factors', type=float_list, default=None,
                   help="also report the priors with every scale multiplied by each of these factors, e.g. 0.5,0.75,1,1.5,2")
    p.add_argument('--draw_priors', type=int, default=0, help="1: write the priors of each feature map over the first case")
    p.add_argument('-o', '--output_dir', type=str, default=r"./insight")
    return p


def check_options(args):
    """Everything that can be refused from the command line alone, before the first GPU call -> (input images, patch
    options, thresholds, scale factors)."""
    input_images = input_images_of(args)
    patch_options = patch_options_of(args)
    segmentation_of(args)
    thr = [float(t) for t in args.threshold]
    if not 1 <= len(thr) <= 2 or any(not 0.0 <= t <= 1.0 for t in thr) or thr != sorted(thr):
        raise ValueError(f"-th takes one threshold or an ascending [lo, hi] band inside [0, 1], got {args.threshold}")
    factors = None if args.scale_factors is None else [float(f) for f in args.scale_factors]
    if factors is not None and (any(not (np.isfinite(f) and f > 0) for f in factors) or len(set(factors)) != len(factors)):
        raise ValueError(f"--scale_factors takes distinct finite factors > 0, got {args.scale_factors}")
    layers = [int(x) for x in args.prediction_layers.split()]
    if not layers or layers != sorted(set(layers)):
        raise ValueError(f"-pl takes ascending distinct layer numbers, got {args.prediction_layers!r}")
    if len(layers) > 8:
        raise ValueError(f"the prior fit report covers at most 8 prediction layers, got {len(layers)}")
    if args.scales and sorted(int(k) for k in args.scales) != layers:
        raise ValueError(f"-sc must name exactly the layers of -pl ({layers}), got {sorted(args.scales)}")
    return input_images, patch_options, thr, factors


def gather_ground_truth(args, input_images, patch_options):
    """-> (true boxes per image, voxels per image, input size, subject of the first image).  The example data set gives its
    volumes as they are; clinical cases are fitted to ``--spatial_size`` (``case_boxes``: the mask alone is loaded), or, with
    ``--patch_size``, cut into the tiles of ``view_plan`` (the validation set of patch training)."""
    from .datasets import ExampleDataset, LesionsDataModule, _LesionTiles
    stage = "predict_train" if args.predict_subset == "train" else "predict"
    boxes, voxels = [], []
    if args.data_module == "lesions":
        module = LesionsDataModule(data_dir=args.dataset_path, centers=tuple(args.centers), batch_size=1,
                                   input_images=input_images, segmentation=segmentation_of(args),
                                   num_workers=args.num_workers, percentage=args.percentage,
                                   spatial_size=tuple(args.spatial_size), **patch_options)
        module.setup(stage=stage)
        cases = module.predict_dataset
        if not len(cases):
            raise RuntimeError("prior fit: no case")
        first = cases.subjects[0]
        first = first if isinstance(first, str) else "_".join(first)
        if patch_options:
            size = tuple(int(v) for v in patch_options["patch_size"])
            tiles = _LesionTiles(cases, size, patch_options["tile_margin"])
            for k in range(len(tiles)):
                boxes.append(tiles[k]["boxes"])
        else:
            size = tuple(int(v) for v in args.spatial_size)
            for pos in range(len(cases)):
                boxes.append(cases.case_boxes(pos, fit=True)[0])
        voxels = [size[0] * size[1] * size[2]] * len(boxes)
        return boxes, voxels, size, first
    ds = ExampleDataset(n_classes=1, percentage=args.percentage, cache=False, num_workers=args.num_workers, objects="multiple",
                        batch_size=1, data_dir=args.dataset_path, dataset_name=args.dataset_name)
    ds.setup(stage=stage)
    size = first = None
    for batch in ds._loader(ds.predict_dataset, False, BATCH):
        boxes.extend(batch["boxes"])
        voxels.extend(batch_voxels(batch))
        if size is None:
            size, first = tuple(int(v) for v in batch["img"].shape[2:]), batch["subject"][0]
    if size is None:
        raise RuntimeError("prior fit: no case")
    return boxes, voxels, size, first


def positive_row(summary):
    """The "all" row at the threshold from which a prior is a positive (the last one)."""
    return summary["thresholds"][-1]["strata"][0]


def suggest(blocks):
    """The factor with the fewest orphaned, then the most matchable lesions (then the one nearest 1)."""
    return min(blocks, key=lambda b: (positive_row(b["fit"])["orphaned"], -positive_row(b["fit"])["matchable"],
                                      abs(np.log(b["factor"]))))["factor"]


def draw_priors(model, ranges, size, subject, out_dir):
    from .utils import cxcycz_to_xyz, draw_boxes
    for f, (lo, hi) in ranges.items():
        if hi - lo > MAX_DRAWN_PRIORS:
            print(f"feature map {f}: {hi - lo} priors do not fit an int16 overlay, not drawn")
            continue
        b = cxcycz_to_xyz(model.priors_cxcycz[lo:hi]).cpu().numpy()
        inst, _ = draw_boxes(b, np.ones(hi - lo, dtype=np.int64), None, size, "edges")
        np.save(pjoin(out_dir, f"sub-{subject}_prior-boxes_fmap-{f}.npy"), inst)


def insight(args):
    input_images, patch_options, thr, factors = check_options(args)
    from . import utils
    from .ssd3d import LSSD3D
    if not torch.cuda.is_available():
        raise RuntimeError("mslesions3d_amd.insight needs the HIP device (no host fallback)")
    boxes, voxels, size, first = gather_ground_truth(args, input_images, patch_options)
    boxes = utils._prior_fit_boxes(boxes)
    layers = [int(x) for x in args.prediction_layers.split()]
    model = LSSD3D(n_classes=2, input_channels=len(input_images), input_size=size, use_wandb=False,
                   aspect_ratios={l: [1.] for l in layers}, scales={int(k): v for k, v in args.scales.items()},
                   threshold=thr, min_object_size=args.min_object_size, max_object_size=args.max_object_size,
                   boxes_per_location=args.boxes_per_location)
    ranges = model.prior_ranges()
    names = list(ranges.keys())
    edges = args.size_bins or ()
    plan = utils.prepare_prior_fit(boxes)  # the one upload of the ground truth

    def block(factor):
        scales = {f: float(model.scales[f]) * factor for f in names}
        fit = utils.run_prior_fit(plan, model.make_priors(scales), thr, ranges)
        return {"factor": factor, "scales": {str(f): s for f, s in scales.items()},
                "fit": utils.prior_fit_summary(fit, boxes, voxels, edges, thr, shapes=size, scale_names=names)}

    out = {"input_size": list(size), "prediction_layers": layers, "thresholds": thr,
           "boxes_per_location": model.boxes_per_location, "n_priors": int(model.priors_cxcycz.shape[0]),
           "prior_ranges": {str(f): [int(lo), int(hi)] for f, (lo, hi) in ranges.items()}}
    out.update({k: v for k, v in block(1.0).items() if k != "factor"})
    if factors is not None:
        out["sweep"] = [block(f) for f in factors]
        out["suggested"] = suggest(out["sweep"])
    os.makedirs(args.output_dir, exist_ok=True)
    with open(pjoin(args.output_dir, "prior_fit.json"), "w") as f:
        json.dump(out, f, indent=4)
    row = positive_row(out["fit"])
    print(f"{row['lesions']} lesions, {out['n_priors']} priors at threshold {thr[-1]}: {row['matchable']} matchable, "
          f"{row['forced_only']} positive through the force-match only, {row['orphaned']} orphaned")
    if factors is not None:
        print(f"suggested scale factor: {out['suggested']}")
    if args.draw_priors:
        draw_priors(model, ranges, size, first, args.output_dir)
    return out


def main(argv=None):
    return insight(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
