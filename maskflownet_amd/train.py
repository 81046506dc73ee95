"""python -m maskflownet_amd.train CONFIG [--dataset_cfg FILE] --data FILE [--root DIR] ...: the reference's main.py on one MI355X.

The arguments are main.py:28-55's.  CONFIG and --dataset_cfg are PATHS to YAML settings files in the reference's format (the package
ships none), --data is the YAML file of dataset roots, split files and validation index lists, --root the run root
that receives logs/, weights/ and flows/ (default: the working directory).  Three modes: training (default), --valid, --predict
(run.TrainingRun, run.validate_checkpoint, run.predict_checkpoint)."""
import argparse


def parser():
    ap = argparse.ArgumentParser(prog="python -m maskflownet_amd.train", description=__doc__)
    ap.add_argument("config", help="network settings file (MaskFlownet_S.yaml, MaskFlownet.yaml, ...)")
    ap.add_argument("--dataset_cfg", default="chairs.yaml", help="dataset settings file")
    ap.add_argument("--data", default=None, help="YAML file of dataset roots, split files and validation index lists")
    ap.add_argument("--root", default=".", help="run root: logs/, weights/ and flows/ live here")
    ap.add_argument("--seed", type=int, default=0, help="seed of the initial weights, the sampler and the augmenters")
    ap.add_argument("--batch", type=int, default=8, help="batch of validation and prediction")
    ap.add_argument("-s", "--shard", type=int, default=1, help="things3d only: every shard-th sample is loaded")
    ap.add_argument("-g", "--gpu_device", default="0", help="device index (one)")
    ap.add_argument("-c", "--checkpoint", default=None, help="run id prefix, or prefix:steps; by default the run's latest checkpoint")
    ap.add_argument("--clear_steps", action="store_true")
    ap.add_argument("-n", "--network", default="MaskFlownet", help="the pipeline; the class comes from the settings' network.class")
    ap.add_argument("--debug", action="store_true", help="32 samples per set, logs under logs/debug")
    ap.add_argument("--valid", action="store_true", help="validate the checkpoint on Sintel and KITTI")
    ap.add_argument("--predict", action="store_true", help="write the Sintel and KITTI test submissions of the checkpoint")
    ap.add_argument("--resize", default="", help="H,W the network runs at in --valid and --predict")
    return ap


def device_of(gpu_device):
    ids = [s for s in gpu_device.split(",") if s.strip()]
    if len(ids) > 1:
        raise NotImplementedError("--gpu_device %s: this driver runs one device.  The gradient exchange of a multi-device step exists "
                                  "(training.GradientBuckets, Trainer(dist=...)); a multi-process driver on top of it does not" % gpu_device)
    if not ids:
        raise ValueError("--gpu_device: a device index is needed: there is no CPU path")
    return "cuda:%d" % int(ids[0])


def main(argv=None):
    import yaml
    from . import config, run
    args = parser().parse_args(argv)
    if args.network != "MaskFlownet":
        raise NotImplementedError("--network %s (the reference has the one pipeline, 'MaskFlownet')" % args.network)
    device = device_of(args.gpu_device)
    network_cfg = config.load(args.config)
    data = {}
    if args.data is not None:
        with open(args.data) as f:
            data = yaml.safe_load(f) or {}
    resize = [int(s) for s in args.resize.split(",")] if args.resize else None
    if args.valid or args.predict:
        if args.checkpoint is None:
            raise ValueError("--valid and --predict need --checkpoint")
        if args.predict:
            for path in run.predict_checkpoint(network_cfg, data, args.root, args.checkpoint, resize=resize, device=device):
                print(path)
        else:
            run.validate_checkpoint(network_cfg, data, args.root, args.checkpoint, batch=args.batch, resize=resize, device=device)
        return 0
    training_run = run.TrainingRun(network_cfg, config.load(args.dataset_cfg), data, args.root, seed=args.seed, checkpoint=args.checkpoint,
                                   clear_steps=args.clear_steps, debug=args.debug, device=device, shard=args.shard, batch=args.batch,
                                   arguments=dict(vars(args)), screen=True)
    training_run.run()
    training_run.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
