"""Train a scene from images: python gaussian_point_train.py --train_config PATH (the reference's script and YAML format)."""
import argparse

from taichi_3d_gaussian_splatting_amd.GaussianPointTrainer import GaussianPointCloudTrainer

if __name__ == "__main__":
    parser = argparse.ArgumentParser("Train a Gaussian Point Cloud Scene")
    parser.add_argument("--train_config", type=str, required=True)
    parser.add_argument("--gen_template_only", action="store_true", default=False)
    args = parser.parse_args()
    if args.gen_template_only:
        import dataclasses

        import yaml
        with open(args.train_config, "w") as fh:
            yaml.safe_dump(dataclasses.asdict(GaussianPointCloudTrainer.TrainConfig()), fh)
        raise SystemExit(0)
    config = GaussianPointCloudTrainer.TrainConfig.from_yaml_file(args.train_config)
    if config.unknown_keys:
        print("ignored keys of the config:", ", ".join(config.unknown_keys))
    trainer = GaussianPointCloudTrainer(config)
    trainer.train()
