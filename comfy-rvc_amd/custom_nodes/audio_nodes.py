"""ComfyUI audio nodes (drop-in for MergeAudioNode, ProcessAudioNode, AudioBatchValueNode and AudioInfoNode of reference
custom_nodes/audio_nodes.py:54-72, :124-170, :224-347; LoadAudio, PreviewAudio and DownloadAudio stay out: file codecs, ffmpeg, network).

INPUT_TYPES (names, order, defaults, ranges), RETURN_TYPES / RETURN_NAMES / FUNCTION / CATEGORY / OUTPUT_NODE follow the reference; the sample work
runs on the device (lib/audio_fx.py, lib/audio.py::AudioProcessor).

Deviation (MergeAudioNode): the reference writes the merged signal to a flac preview and reads it back through ffmpeg at 44.1 kHz, so its output
is the codec's and the loader's version of the mix.  No codec is available to this build: the node returns the merged signal itself at the merge
rate and only names a preview entry (as RVCNode does), with the VHS_AUDIO thunk producing WAV bytes.
"""
import numpy as np

from ..lib import audio_fx
from ..lib.audio import MAX_INT16, AudioProcessor, audio_to_bytes, get_audio, remix_audio
from .rvc_nodes import MultipleTypeProxy, get_hash, to_audio_dict

CATEGORY = "🌺RVC-Studio/audio"
MERGE_OPTIONS = ["median", "mean", "min", "max"]      # reference custom_nodes/settings/__init__.py:11


def _mono(audio):
    """get_audio's (samples, sr) with the samples as float32 [n]: [n, C] / [C, n] layouts are averaged over the short axis."""
    samples, sr = get_audio(audio)
    samples = np.asarray(samples, dtype=np.float32)
    if samples.ndim > 1:
        samples = samples.mean(axis=int(np.argmin(samples.shape)), dtype=np.float32)
    return samples, int(sr)


class AudioInfoNode:
    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {"audio": (MultipleTypeProxy("AUDIO,VHS_AUDIO"),)}}

    CATEGORY = CATEGORY
    RETURN_TYPES = ("VHS_AUDIO", "AUDIO", "FLOAT", "INT")
    RETURN_NAMES = ("vhs_audio", "audio", "seconds", "sr")
    FUNCTION = "get_info"

    def get_info(self, audio):
        input_audio = get_audio(audio)
        seconds = len(input_audio[0]) / input_audio[1]
        return (lambda: audio_to_bytes(*input_audio), to_audio_dict(*input_audio), float(seconds), int(input_audio[1]))


class MergeAudioNode:
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "audio1": (MultipleTypeProxy("AUDIO,VHS_AUDIO"),),
                "audio2": (MultipleTypeProxy("AUDIO,VHS_AUDIO"),),
            },
            "optional": {
                "sr": (["None", 32000, 40000, 44100, 48000], {"default": "None"}),
                "merge_type": (MERGE_OPTIONS, {"default": "median"}),
                "normalize": ("BOOLEAN", {"default": True}),
                "audio3_opt": (MultipleTypeProxy("AUDIO,VHS_AUDIO"), {"default": None}),
                "audio4_opt": (MultipleTypeProxy("AUDIO,VHS_AUDIO"), {"default": None}),
            },
        }

    RETURN_TYPES = ("VHS_AUDIO", "AUDIO")
    RETURN_NAMES = ("vhs_audio", "audio")
    OUTPUT_NODE = True
    FUNCTION = "merge"
    CATEGORY = CATEGORY

    def merge(self, audio1, audio2, sr="None", merge_type="median", normalize=False, audio3_opt=None, audio4_opt=None):
        input_audios = [_mono(audio) for audio in [audio1, audio2, audio3_opt, audio4_opt] if audio is not None]
        widget_id = get_hash(*[audio_to_bytes(*audio) for audio in input_audios], sr, merge_type, normalize)
        merged_sr = min(rate for _, rate in input_audios) if sr == "None" else int(sr)
        # every track at the merge rate (resample_audio on the device), peak-normalised when asked, limited to 0.95: remix_audio as in the reference
        tracks = [remix_audio(audio, merged_sr, norm=normalize)[0] for audio in input_audios]
        merged = audio_fx.merge_tracks(tracks, merge_type).cpu().numpy()
        merged_audio = (merged, merged_sr)
        ui = {"preview": [{"filename": f"{widget_id}.wav", "type": "temp", "subfolder": "preview", "widgetId": widget_id}]}
        return {"ui": ui, "result": (lambda: audio_to_bytes(*merged_audio), to_audio_dict(*merged_audio))}


class ProcessAudioNode:
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "normalize": ("BOOLEAN", {"default": True}),
                "threshold_silence": ("BOOLEAN", {"default": True}),
                "dynamic_threshold": ("BOOLEAN", {"default": True}),
            },
            "optional": {
                "audio": (MultipleTypeProxy("AUDIO,VHS_AUDIO"), {"default": None}),
                "dynamic_threshold_sample_size": ("INT", {"default": 4000, "min": 160, "max": 48000, "step": 160}),
                "dynamic_threshold_multiplier": ("FLOAT", {"default": 2., "min": 1.5, "step": .1}),
                "dynamic_threshold_fill_method": (["median", "interpolation"], {"default": "median"}),
                "dynamic_threshold_kernel_size": ("INT", {"default": 5, "min": 3, "step": 2}),
                "silence_threshold_db": ("INT", {"default": -50, "min": -120, "max": 0}),
                "normalize_threshold_db": ("INT", {"default": -1, "min": -10, "max": 0}),
            },
        }

    RETURN_TYPES = ("AUDIO_PROCESSOR", "VHS_AUDIO", "AUDIO")
    RETURN_NAMES = ("audio_processor", "vhs_audio", "audio")
    CATEGORY = CATEGORY
    FUNCTION = "process_audio"

    def process_audio(self, normalize, threshold_silence, dynamic_threshold, audio=None, dynamic_threshold_sample_size=16000,
                      dynamic_threshold_multiplier=2.0, dynamic_threshold_fill_method="median", dynamic_threshold_kernel_size=5,
                      silence_threshold_db=-50, normalize_threshold_db=-1):
        audio_processor = AudioProcessor(normalize=normalize, threshold_silence=threshold_silence, dynamic_threshold=dynamic_threshold,
                                         sample_size=dynamic_threshold_sample_size, multiplier=dynamic_threshold_multiplier,
                                         fill_method=dynamic_threshold_fill_method, kernel_size=dynamic_threshold_kernel_size,
                                         silence_threshold_db=silence_threshold_db, normalize_threshold_db=normalize_threshold_db)
        if audio is None:
            vhs_audio = comfy_audio = audio
        else:
            output_audio = audio_processor(audio)
            vhs_audio = lambda: audio_to_bytes(*output_audio)   # noqa: E731
            comfy_audio = to_audio_dict(*output_audio)
        return (audio_processor, vhs_audio, comfy_audio)


class AudioBatchValueNode:
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "audio": (MultipleTypeProxy("AUDIO,VHS_AUDIO"),),
                "num_segments": ("INT", {"default": 2, "min": 2, "max": 256, "step": 1}),
                "output_min": ("FLOAT", {"default": 0., "min": -1000., "max": 1000., "step": .01}),
                "output_max": ("FLOAT", {"default": 1., "min": 0., "max": 1000., "step": .01}),
                "norm": (["scale", "tanh", "sigmoid"], {"default": "scale"}),
            },
            "optional": {
                "silence_threshold": ("INT", {"default": 1000, "min": 1, "max": MAX_INT16, "step": 1}),
                "duration_list": ("INT", {"default": 0, "min": 0, "forceInput": True}),
                "print_output": ("BOOLEAN", {"default": False}),
                "inverse": ("BOOLEAN", {"default": False}),
            },
        }

    RETURN_TYPES = ("FLOAT", "INT", "INT")
    RETURN_NAMES = ("FLOAT", "INT", "num_values")
    FUNCTION = "get_frame_weights"
    CATEGORY = CATEGORY

    @staticmethod
    def get_rms(audio):     # root mean squared of an audio segment (host; the node itself takes the segment sums from the device)
        return np.sqrt(np.nanmean(audio ** 2))

    @staticmethod
    def to_int16(samples, max_volume=.95):
        """remix_audio(audio, norm=True, to_int16=True) as the reference evaluates it (lib/audio.py:144-163 with librosa.util.normalize): float32
        samples, several channels averaged, divided by their FLOAT64 peak (librosa takes the magnitudes as float64, so everything after it is
        float64 - this package's remix_audio keeps float32 there, which moves a few int16 values by one), limited to max_volume, scaled to int16."""
        a = np.array(samples, dtype="float32")
        if a.ndim > 1:
            a = np.nanmean(a, axis=0)
        peak = np.abs(a).astype(float).max()
        a = a / (1.0 if peak < np.finfo(np.float32).tiny else peak)
        audio_max = np.abs(a).max() / max_volume
        if audio_max > 1:
            a = a / audio_max
        return np.clip(a * MAX_INT16, a_min=1 - MAX_INT16, a_max=MAX_INT16 - 1).astype("int16")

    @staticmethod
    def segment_rms(audio_i16, num_values, silence_threshold):
        """get_rms of every np.array_split segment of audio / silence_threshold: the exact int64 segment sums come from the device in one launch;
        the square root and the division stay on the host (float64)."""
        energy = audio_fx.segment_energy(audio_i16, num_values)
        lens = np.diff(audio_fx.split_bounds(np.asarray(audio_i16).size, num_values))
        return np.sqrt(energy.astype(np.float64) / lens) / silence_threshold

    def get_frame_weights(self, audio, num_segments, output_min, output_max, norm, silence_threshold=1000, duration_list=0, print_output=False,
                          inverse=False):
        assert output_max >= output_min, f"{output_max=} must be greater or equal to {output_min=}!"
        audio = self.to_int16(get_audio(audio)[0])
        num_values = int(num_segments)
        audio_rms = np.nan_to_num(self.segment_rms(audio.flatten(), num_values, silence_threshold), nan=0)
        audio_zscore = (audio_rms - audio_rms.mean()) / audio_rms.std()
        output_range = output_max - output_min
        if norm == "tanh":
            x_norm = np.tanh(audio_zscore)                              # -1 to 1
            if inverse:
                x_norm *= -1
            x_norm = (x_norm * output_range + output_max + output_min) / 2
        elif norm == "sigmoid":
            x_norm = 1. / (1. + np.exp(-audio_zscore))                  # 0 to 1
            if inverse:
                x_norm = 1 - x_norm
            x_norm = x_norm * output_range + output_min
        else:
            x_min = audio_zscore.min()
            x_norm = (audio_zscore - x_min) / (audio_zscore.max() - x_min)   # 0 to 1
            if inverse:
                x_norm = 1 - x_norm
            x_norm = x_norm * output_range + output_min
        if print_output:
            print(f"{audio_rms.min()=} {audio_rms.max()=} {audio_rms.mean()=} {len(audio_rms)=}")
            print(f"{x_norm.min()=} {x_norm.max()=} {x_norm.mean()=} {len(x_norm)=}")
        if isinstance(duration_list, list):
            x_norm = [list(part) for part in np.array_split(x_norm, np.cumsum(duration_list))]
            x_norm_int = [list(map(int, part)) for part in x_norm]
        else:
            x_norm_int = map(int, x_norm)
        return (list(x_norm), list(x_norm_int), num_values)


NODE_CLASS_MAPPINGS = {
    "MergeAudioNode": MergeAudioNode,
    "AudioBatchValueNode": AudioBatchValueNode,
    "ProcessAudioNode": ProcessAudioNode,
    "AudioInfoNode": AudioInfoNode,
}
# (no display-name entries: ComfyUI shows the class name for a node without one, and the display-name table stays the set of the inference
# nodes - see the note at the end of rvc_nodes.py)
NODE_DISPLAY_NAME_MAPPINGS = {}
