"""The part of the reference's lib/train/utils.py that the data loaders and the trainer's checkpoints need: WAV and file-list readers, the HParams container,
save_checkpoint / load_checkpoint / latest_checkpoint_path."""
import glob
import json
import os

import numpy as np
import torch


def load_wav_to_torch(full_path):
    """(float32 tensor of the samples as stored - no scaling, the training clips are IEEE-float WAVs - , sampling rate); lib/train/utils.py:247-249."""
    from scipy.io import wavfile   # noqa: PLC0415
    sampling_rate, data = wavfile.read(full_path)
    return torch.from_numpy(np.asarray(data).astype(np.float32)), sampling_rate


def load_filepaths_and_text(filename, split="|"):
    """The rows of a filelist.txt, split at `split` (lib/train/utils.py:252-255)."""
    with open(filename, encoding="utf-8") as f:
        return [line.strip().split(split) for line in f]


class HParams:
    """Attribute / item access over a (nested) dict of settings (lib/train/utils.py:429-460)."""

    def __init__(self, **kwargs):
        for k, v in kwargs.items():
            self[k] = HParams(**v) if isinstance(v, dict) else v

    def keys(self):
        return self.__dict__.keys()

    def items(self):
        return self.__dict__.items()

    def values(self):
        return self.__dict__.values()

    def __len__(self):
        return len(self.__dict__)

    def __getitem__(self, key):
        return getattr(self, key)

    def __setitem__(self, key, value):
        setattr(self, key, value)

    def __contains__(self, key):
        return key in self.__dict__

    def __repr__(self):
        return repr(self.__dict__)


def get_hparams_from_file(config_path):
    """HParams of a configs/*.json file (lib/train/utils.py:380-386)."""
    with open(config_path, "r") as f:
        return HParams(**json.load(f))


def save_checkpoint(model, optimizer, learning_rate, iteration, checkpoint_path, **kwargs):
    """Writes the trainer's G_*.pth / D_*.pth (lib/train/utils.py:119-134): {"model": model.state_dict(), "iteration", "optimizer": optimizer.state_dict(),
    "learning_rate", "kwargs"} through torch.save.  With a trainable discriminator net and lib.train.optim.AdamW the file is one the reference's trainer
    resumes from: host float32 tensors under the reference's names, the optimizer state in torch.optim.AdamW's format."""
    model = getattr(model, "module", model)
    torch.save({"model": model.state_dict(), "iteration": iteration, "optimizer": optimizer.state_dict(), "learning_rate": learning_rate, "kwargs": kwargs},
               checkpoint_path)


def load_checkpoint(checkpoint_path, model, optimizer=None, load_opt=1):
    """(model, optimizer, learning_rate, iteration, kwargs) from a file of save_checkpoint or of the reference's trainer (lib/train/utils.py:76-116).  A tensor
    the checkpoint lacks, or holds in another shape, keeps the model's own value where the model can tell it (a net with state_dict()); the optimizer state is
    loaded when an optimizer is given and load_opt == 1."""
    if not os.path.isfile(checkpoint_path):
        raise FileNotFoundError(checkpoint_path)
    ckpt = torch.load(checkpoint_path, map_location="cpu")
    saved = ckpt["model"]
    target = getattr(model, "module", model)
    try:
        own = target.state_dict()
    except (AttributeError, ValueError, AssertionError):         # a net that keeps no parameters, or is not loaded yet: take the checkpoint as it is
        own = None
    if own is None:
        merged = saved
    else:
        merged = {}
        for name, value in own.items():
            if name in saved and tuple(saved[name].shape) == tuple(value.shape):
                merged[name] = saved[name]
            else:
                print(f"{name} is not in the checkpoint (or has another shape): kept")
                merged[name] = value
    target.load_state_dict(merged, strict=False)
    if optimizer is not None and load_opt == 1:
        optimizer.load_state_dict(ckpt["optimizer"])
    return model, optimizer, ckpt["learning_rate"], ckpt["iteration"], ckpt.get("kwargs", {})


def latest_checkpoint_path(dir_path, regex="G_*.pth"):
    """The file matching `regex` under dir_path whose name carries the largest number (lib/train/utils.py:182-187: all digits of the path, read as one)."""
    files = glob.glob(os.path.join(dir_path, regex))
    if not files:
        raise FileNotFoundError(f"no {regex} under {dir_path}")
    return max(files, key=lambda f: int("".join(ch for ch in f if ch.isdigit()) or 0))
