"""Silent and Normalize on the device (mirror of reference lib/karafan/audio_utils.py:89-167; KaraFan, MIT License - Copyright (c) 2023 Captain
FLAM & Jarredou).  Signatures are the reference's; numpy arrays come back as numpy arrays of the input's shape, CUDA tensors stay on the device
(lib/audio.py::AudioProcessor chains the steps that way).

Deviation: Silent takes ONE channel ([n] or [1, n]).  The reference's own slicing `audio[:, i:(i + window_frame)]` of a [channels, n] array works,
but its caller hands it the transposed layout of get_audio, where that slice indexes the wrong axis; this build down-mixes before the gate, as
get_audio / remix_audio users do everywhere else, and raises on a 2-D input with more than one row.
"""
import numpy as np

from .. import audio_fx


def _mono(audio, what):
    shape = tuple(audio.shape)
    if len(shape) > 2 or (len(shape) == 2 and shape[0] != 1):
        raise ValueError(f"{what}: one channel ([n] or [1, n]) is supported, got shape {shape} - down-mix first")
    return shape


def Normalize(audio, threshold_dB=-1.0):
    """DC removed (mean over all samples), peak at 10^(threshold_dB / 20); a peak of 0 stays 0."""
    on_device = hasattr(audio, "is_cuda")
    shape = tuple(audio.shape)
    y = audio_fx.peak_normalize(audio if on_device else np.asarray(audio, dtype=np.float32), threshold_dB)
    return y.reshape(shape) if on_device else y.cpu().numpy().reshape(shape)


def Silent(audio_in, sample_rate, threshold_dB=-50):
    """Stretches of more than 1 s whose 0.5 s windows all stay below threshold_dB are zeroed, with 0.3 s fades at their edges."""
    on_device = hasattr(audio_in, "is_cuda")
    shape = _mono(audio_in, "Silent")
    y = audio_fx.silence_gate(audio_in if on_device else np.asarray(audio_in, dtype=np.float32), sample_rate, threshold_dB)
    return y.reshape(shape) if on_device else y.cpu().numpy().reshape(shape)
