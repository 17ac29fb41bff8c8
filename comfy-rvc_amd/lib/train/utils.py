"""The part of the reference's lib/train/utils.py that the data loaders need: WAV and file-list readers and the HParams container."""
import json

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
