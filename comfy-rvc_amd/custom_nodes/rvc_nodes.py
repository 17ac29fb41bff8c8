"""ComfyUI node surface of the RVC inference path and of dataset preparation (drop-in for the four inference nodes of reference
custom_nodes/rvc_nodes.py:44-206 and for RVCProcessDatasetNode, :208-349; the training nodes, downloads and audio codecs are out of scope).

Node names, categories, INPUT_TYPES / RETURN_TYPES / FUNCTION and the tuple protocol between nodes follow the reference:
  LoadPitchExtractionParams -> ('PITCH_EXTRACTION',)   = the kwargs dict itself
  LoadHubertModel           -> ('HUBERT_MODEL',)       = zero-argument thunk returning the model
  LoadRVCModelNode          -> ('RVC_MODEL', 'STRING') = thunk returning get_vc(...)'s dict, model name
  RVCNode.convert           -> {"ui": ..., "result": (VHS_AUDIO thunk, AUDIO dict {"waveform": [1, N, C], "sample_rate"})}
  RVCProcessDatasetNode     -> ('RVC_DATASET_PIPE',)   = dict(sample_rate, dataset_dir, name, training_files, if_f0, pitch_extraction_params, hubert_model)
The reference re-loads the weights on every execution because the thunks are not cached (rvc_nodes.py:191-192); here they
are memoised per (path, mtime) so repeated graph runs keep the weights resident in HBM.
"""
import hashlib
import os

import numpy as np
import torch

from ..config import config
from ..lib import BASE_DIR, BASE_MODELS_DIR
from ..lib.audio import audio_to_bytes, get_audio
from ..lib.model_utils import load_hubert
from ..vc_infer_pipeline import get_vc, vc_single

CATEGORY = "🌺RVC-Studio/rvc"
PITCH_EXTRACTION_OPTIONS = ["crepe", "mangio-crepe", "rmvpe", "rmvpe+"]
SUPPORTED_AUDIO = ["mp3", "flac", "wav"]
SR_MAP = {"32k": 32000, "40k": 40000, "48k": 48000}
try:                                            # inside ComfyUI: its input / output folders, like the reference
    import folder_paths
    INPUT_DIR, OUTPUT_DIR = folder_paths.get_input_directory(), folder_paths.get_output_directory()
except ImportError:
    INPUT_DIR, OUTPUT_DIR = os.path.join(BASE_DIR, "input"), os.path.join(BASE_DIR, "output")


class MultipleTypeProxy(str):
    """Socket type that matches any of several comma-separated ComfyUI types (reference custom_nodes/utils.py:32-41)."""

    def __eq__(self, other):
        mine, theirs = set(self.split(",")), set(str(other).split(","))
        return bool(mine & theirs) or str(self) == "*"

    def __ne__(self, other):
        return not self.__eq__(other)

    __hash__ = str.__hash__


def to_audio_dict(audio, sr):
    """ndarray [N] or [C, N] -> {"waveform": tensor [1, N, C], "sample_rate"} (reference custom_nodes/audio_nodes.py:17-20)."""
    audio = np.atleast_2d(audio)
    return dict(waveform=torch.from_numpy(audio.reshape((-1, audio.shape[0]))).unsqueeze(0), sample_rate=sr)


def _list_models(folder, exts):
    root = os.path.join(BASE_MODELS_DIR, folder)
    if not os.path.isdir(root):
        return []
    return sorted(f for f in os.listdir(root) if f.rsplit(".", 1)[-1] in exts)


_memo = {}


def _memoised(kind, path, loader, extra=None):
    mt = lambda f: os.path.getmtime(f) if f and os.path.isfile(f) else None   # noqa: E731
    key = (kind, path, mt(path), extra, mt(extra))
    if key not in _memo:
        _memo[key] = loader()
    return _memo[key]


def train_index(dataset_dir, sr, name):
    """RVCTrainModelNode.train_index of the reference (custom_nodes/rvc_nodes.py:500-554) as a plain function - the training NODE stays out of
    scope, a graph or the reference's node can call this: the HuBERT features under `dataset_dir/3_feature768` become
    `BASE_MODELS_DIR/RVC/.index/{name}_v2_{sr}_{md5(dataset_dir, sr, name)}.index`, trained on the GPU (lib/feature_index.py::train_index).
    An existing file is kept; returns the path, or None when the build failed (as the reference does)."""
    from ..lib.feature_index import train_index as build
    key = hashlib.md5("".join(str(v) for v in (dataset_dir, sr, name)).encode()).hexdigest()      # reference lib/utils.py::get_hash
    index_file = os.path.join(BASE_MODELS_DIR, "RVC", ".index", f"{name}_v2_{sr}_{key}.index")
    try:
        if not os.path.isfile(index_file):
            os.makedirs(os.path.dirname(index_file), exist_ok=True)
            build(os.path.join(dataset_dir, "3_feature768"), index_file)
            print(f"saved index file to {index_file}")
        return index_file
    except Exception as e:   # noqa: BLE001 - the reference reports and returns None
        print(f"Failed to train index: {e}")
    return None


class LoadPitchExtractionParams:
    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {
            "f0_method": (PITCH_EXTRACTION_OPTIONS, {"default": "rmvpe"}),
            "f0_autotune": ("BOOLEAN",),
            "index_rate": ("FLOAT", {"default": .75, "min": 0., "max": 1., "step": .01}),
            "resample_sr": ([0, 16000, 32000, 40000, 44100, 48000], {"default": 0}),
            "rms_mix_rate": ("FLOAT", {"default": 0.25, "min": 0., "max": 1., "step": .01}),
            "protect": ("FLOAT", {"default": 0.25, "min": 0., "max": .5, "step": .01}),
            "crepe_hop_length": ("INT", {"default": 160, "min": 16, "max": 512, "step": 16}),
        }}

    RETURN_TYPES = ("PITCH_EXTRACTION",)
    RETURN_NAMES = ("pitch_extraction_params",)
    CATEGORY = CATEGORY
    FUNCTION = "load_params"

    def load_params(self, **params):
        return (params,)


class LoadHubertModel:
    @classmethod
    def INPUT_TYPES(cls):
        models = sorted(set(["content-vec-best.safetensors"] + _list_models(".", ("pt", "safetensors"))))
        return {"required": {"model": (models, {"default": "content-vec-best.safetensors"})}}

    RETURN_TYPES = ("HUBERT_MODEL",)
    RETURN_NAMES = ("hubert_model",)
    CATEGORY = CATEGORY
    FUNCTION = "load_model"

    def load_model(self, model):
        path = os.path.join(BASE_MODELS_DIR, model)
        return (lambda: _memoised("hubert", path, lambda: load_hubert(path, config=config)),)


class LoadRVCModelNode:
    @classmethod
    def INPUT_TYPES(cls):
        models = [f"RVC/{m}" for m in _list_models("RVC", ("pth",))] or [""]
        # faiss .index files (readable when faiss is installed) and big_npy .npy matrices (the vectors the index is built from)
        index = [""] + [f"RVC/.index/{m}" for m in _list_models(os.path.join("RVC", ".index"), ("index", "npy"))]
        return {"required": {"model": (models, {"default": models[0]})}, "optional": {"index": (index, {"default": ""})}}

    RETURN_TYPES = ("RVC_MODEL", "STRING")
    RETURN_NAMES = ("model", "model_name")
    CATEGORY = CATEGORY
    FUNCTION = "load_model"

    def load_model(self, model, index=""):
        path = os.path.join(BASE_MODELS_DIR, os.path.dirname(model), os.path.basename(model))
        file_index = os.path.join(BASE_MODELS_DIR, os.path.dirname(model), ".index", os.path.basename(index)) if index else None
        return (lambda: _memoised("rvc", path, lambda: get_vc(path, file_index), extra=file_index), os.path.basename(model).split(".")[0])


class _ByteLRU:
    """Result cache of RVCNode bounded by BYTES (upstream caches on disk by file name, reference rvc_nodes.py:176-183; a long-lived ComfyUI server would
    otherwise keep 2.4 MB per distinct 30 s conversion forever): least recently used entries go first, one entry larger than the bound is not kept."""

    def __init__(self, max_bytes):
        from collections import OrderedDict
        self.max_bytes, self.bytes, self._d = int(max_bytes), 0, OrderedDict()

    def __contains__(self, key):
        return key in self._d

    def __len__(self):
        return len(self._d)

    def get(self, key):
        self._d.move_to_end(key)
        return self._d[key]

    def put(self, key, value):
        n = int(np.asarray(value[0]).nbytes)
        if key in self._d:
            self.bytes -= int(np.asarray(self._d.pop(key)[0]).nbytes)
        if n > self.max_bytes:
            return
        self._d[key] = value
        self.bytes += n
        while self.bytes > self.max_bytes:
            _, old = self._d.popitem(last=False)
            self.bytes -= int(np.asarray(old[0]).nbytes)


class RVCNode:
    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {
            "audio": (MultipleTypeProxy("AUDIO,VHS_AUDIO"),),
            "model": ("RVC_MODEL",),
            "hubert_model": ("HUBERT_MODEL",),
            "pitch_extraction_params": ("PITCH_EXTRACTION",),
            "f0_up_key": ("INT", {"default": 0, "min": -14, "max": 14, "step": 1, "display": "slider"}),
        }, "optional": {"format": (SUPPORTED_AUDIO, {"default": "flac"}), "use_cache": ("BOOLEAN", {"default": True})}}

    OUTPUT_NODE = True
    RETURN_TYPES = ("VHS_AUDIO", "AUDIO")
    FUNCTION = "convert"
    CATEGORY = CATEGORY
    CACHE_BYTES = 256 << 20                        # ~ 100 conversions of 30 s at 40 kHz int16
    _cache = _ByteLRU(CACHE_BYTES)

    def convert(self, audio, model, hubert_model, pitch_extraction_params, f0_up_key, format="flac", use_cache=True):
        input_audio = get_audio(audio)
        voice_model = model()
        feature_model = hubert_model()
        h = hashlib.md5()
        for part in (feature_model.__class__.__name__, voice_model.get("model_name"), str(voice_model.get("file_index")), f0_up_key,
                     sorted(pitch_extraction_params.items())):
            h.update(str(part).encode())
        h.update(np.ascontiguousarray(input_audio[0]).tobytes())
        widget_id = h.hexdigest()
        if use_cache and widget_id in self._cache:
            output_audio = self._cache.get(widget_id)
        else:
            output_audio = vc_single(hubert_model=feature_model, input_audio=input_audio, f0_up_key=f0_up_key, **voice_model,
                                     **pitch_extraction_params)
            if output_audio is None:
                raise RuntimeError("voice conversion failed (vc_single returned None; see the message printed above)")
            if use_cache:
                self._cache.put(widget_id, output_audio)
        wav, sr = output_audio
        audio_name = f"{widget_id}.{format}"
        ui = {"preview": [{"filename": audio_name, "type": "temp", "subfolder": "preview", "widgetId": widget_id}]}
        # VHS_AUDIO = thunk returning the encoded stream (reference rvc_nodes.py:206: `lambda: audio_to_bytes(*output_audio)`, always WAV:
        # PCM_16 for the int16 result).  `format` only names the preview / cache file upstream; no file is written here (file codecs are
        # out of scope), so flac / mp3 previews are not produced.
        return {"ui": ui, "result": (lambda: audio_to_bytes(wav, sr), to_audio_dict(wav, sr))}


def get_hash(*args, **kwargs):
    """reference lib/utils.py:19-20"""
    return hashlib.md5("".join([str(data) for data in args] + list(kwargs.values())).encode()).hexdigest()


def extract_zip_without_structure(zip_path, extract_to):
    """Every file of the archive directly under extract_to, directories dropped (reference custom_nodes/settings/downloader.py:105-125)."""
    import zipfile
    os.makedirs(extract_to, exist_ok=True)
    with zipfile.ZipFile(zip_path, "r") as z:
        for member in z.namelist():
            filename = os.path.basename(member)
            if filename:
                with z.open(member) as src, open(os.path.join(extract_to, filename), "wb") as dst:
                    dst.write(src.read())
    return os.listdir(extract_to)


class RVCProcessDatasetNode:
    @classmethod
    def INPUT_TYPES(cls):
        dataset_path = os.path.join(INPUT_DIR, "datasets")
        os.makedirs(dataset_path, exist_ok=True)
        datasets = [""] + sorted(d for d in os.listdir(dataset_path) if d.endswith("zip"))
        cpus = os.cpu_count() or 1
        return {"required": {
            "model_name": ("STRING", {"default": ""}),
            "dataset": (datasets, {"default": ""}),
            "hubert_model": ("HUBERT_MODEL",),
        }, "optional": {
            "pitch_extraction_params": ("PITCH_EXTRACTION", {"default": {}}),
            "sr": (["32k", "40k", "48k"], {"default": "40k"}),
            "n_threads": ("INT", {"default": 1, "min": 1, "max": cpus}),      # partitions the file list only: one process, one device
            "period": ("FLOAT", {"default": 3., "min": 1., "max": 10., "step": .1}),
            "overlap": ("FLOAT", {"default": .3, "min": .1, "max": 1., "step": .1}),
            "max_volume": ("FLOAT", {"default": .99, "min": .1, "max": 1., "step": .01}),
            "mute_ratio": ("FLOAT", {"default": .0, "min": .0, "max": .5, "step": .01}),
            "audio_processor": ("AUDIO_PROCESSOR",),
        }}

    RETURN_TYPES = ("RVC_DATASET_PIPE",)
    RETURN_NAMES = ("rvc_dataset_pipe",)
    FUNCTION = "process"
    CATEGORY = CATEGORY

    @staticmethod
    def _mute_set(dataset_dir, sr, hubert, f0_method, crepe_hop_length):
        """3 s of silence as a training clip under dataset_dir/mute, in the layout of the set the reference ships in its own dataset/mute (which
        this build does not carry): 0_gt_wavs/mute{sr}.wav, 1_16k_wavs/mute.wav and the feature dump of the latter."""
        from scipy.io import wavfile
        from ..preprocessing_utils import FeatureInput
        mute = os.path.join(dataset_dir, "mute")
        dirs = {k: os.path.join(mute, k) for k in ("0_gt_wavs", "1_16k_wavs", "2a_f0", "2b-f0nsf", "3_feature768")}
        for d in dirs.values():
            os.makedirs(d, exist_ok=True)
        gt, w16 = os.path.join(dirs["0_gt_wavs"], f"mute{sr}.wav"), os.path.join(dirs["1_16k_wavs"], "mute.wav")
        if not os.path.isfile(gt):
            wavfile.write(gt, SR_MAP[sr], np.zeros(3 * SR_MAP[sr], dtype=np.float32))
        if not os.path.isfile(w16):
            wavfile.write(w16, 16000, np.zeros(3 * 16000, dtype=np.float32))
        out = (os.path.join(dirs["2a_f0"], "mute.wav"), os.path.join(dirs["2b-f0nsf"], "mute.wav"), os.path.join(dirs["3_feature768"], "mute"))
        fi = FeatureInput(hubert, f0_method, mute, version="v2", if_f0=bool(f0_method), hop_size=crepe_hop_length)
        fi.go([(w16,) + out], shard=False)
        files = [gt, out[2] + ".npy"] + ([out[0] + ".npy", out[1] + ".npy"] if f0_method else [])
        missing = [f for f in files if not os.path.isfile(f)]
        assert not missing, f"Failed to build the mute set: {missing}"
        return files

    def process(self, model_name, dataset, hubert_model, pitch_extraction_params={}, sr="40k", n_threads=1, period=3., overlap=.3, max_volume=1.,
                mute_ratio=.0, audio_processor=None):
        """`dataset`: a .zip under INPUT_DIR/datasets (extracted flat next to it) or a folder of recordings (absolute, or under INPUT_DIR/datasets)."""
        from ..preprocessing_utils import extract_features_trainset, preprocess_trainset
        assert model_name, "Please provide a model name!"
        assert dataset, "Please upload a dataset!"
        f0_method = pitch_extraction_params.get("f0_method", "")
        cached_params = [dataset, period, overlap, max_volume, mute_ratio, sr, f0_method, audio_processor]
        crepe_hop_length = pitch_extraction_params.get("crepe_hop_length", 160)
        if "crepe" in f0_method:
            cached_params.append(crepe_hop_length)
        cache_name = get_hash(*cached_params)
        dataset_dir = os.path.join(OUTPUT_DIR, "dataset", cache_name)
        os.makedirs(dataset_dir, exist_ok=True)
        filelist_path = os.path.join(dataset_dir, "filelist.txt")
        if not os.path.isfile(filelist_path):
            dataset_path = os.path.join(INPUT_DIR, "datasets")
            if dataset.endswith("zip"):
                input_dir = os.path.join(dataset_path, os.path.basename(dataset).split(".")[0])
                zip_path = dataset if os.path.isabs(dataset) else os.path.join(dataset_path, dataset)
                assert len(extract_zip_without_structure(zip_path, input_dir)), "Failed to extract zip file..."
            else:
                input_dir = dataset if os.path.isdir(dataset) else os.path.join(dataset_path, dataset)
            assert os.path.isdir(input_dir), f"dataset folder not found: {input_dir}"
            assert preprocess_trainset(input_dir, SR_MAP[sr], n_threads, dataset_dir, audio_processor, period, overlap, max_volume), \
                "Failed to preprocess audio..."
            hubert = hubert_model()
            assert extract_features_trainset(hubert, dataset_dir, n_p=n_threads, f0method=f0_method, device=config.device, if_f0=bool(f0_method),
                                             version="v2", crepe_hop_length=crepe_hop_length), "Failed to extract features..."
            gt_wavs_dir, feature_dir = os.path.join(dataset_dir, "0_gt_wavs"), os.path.join(dataset_dir, "3_feature768")
            f0_dir, f0nsf_dir = os.path.join(dataset_dir, "2a_f0"), os.path.join(dataset_dir, "2b-f0nsf")
            stems = lambda d: set(os.path.splitext(name)[0] for name in os.listdir(d))   # noqa: E731
            names = stems(feature_dir) & stems(f0_dir) & stems(f0nsf_dir) if f0_method else stems(feature_dir)
            opt, missing_data = [], []
            for name in sorted(names):
                gt_name = name.split(",")[-1]
                gt_file = os.path.join(gt_wavs_dir, gt_name)
                if not os.path.isfile(gt_file):
                    print(f"{gt_name} not found!")
                    missing_data.append(gt_name)
                    continue
                cols = [gt_file, os.path.join(feature_dir, f"{name}.npy")]
                if f0_method:
                    cols += [os.path.join(f0_dir, f"{name}.npy"), os.path.join(f0nsf_dir, f"{name}.npy")]
                opt.append("|".join(cols + [str(0)]))
            assert len(missing_data) == 0, f"missing ground truth data: {len(opt)=}, {len(missing_data)=}"
            mute = self._mute_set(dataset_dir, sr, hubert, f0_method, crepe_hop_length)
            mute_line = "|".join(mute + [str(0)])
            opt += [mute_line] * max(2, int(len(opt) * mute_ratio))
            np.random.shuffle(opt)
            with open(filelist_path, "w") as f:
                f.write("\n".join(opt))
            print("write filelist done")
        return (dict(sample_rate=sr, dataset_dir=dataset_dir, name=model_name, training_files=filelist_path, if_f0=bool(f0_method),
                     pitch_extraction_params=pitch_extraction_params, hubert_model=hubert_model),)


NODE_CLASS_MAPPINGS = {
    "LoadRVCModelNode": LoadRVCModelNode,
    "RVCNode": RVCNode,
    "LoadHubertModel": LoadHubertModel,
    "LoadPitchExtractionParams": LoadPitchExtractionParams,
    "RVCProcessDatasetNode": RVCProcessDatasetNode,
}
NODE_DISPLAY_NAME_MAPPINGS = {
    "LoadRVCModelNode": "🌺Load RVC Model",
    "RVCNode": "🌺Voice Changer",
    "LoadHubertModel": "🌺Load Hubert Model",
    "LoadPitchExtractionParams": "🌺Load Pitch Extraction Params",
}
# (RVCProcessDatasetNode is registered above under its class name, which ComfyUI also shows for a node without an entry here: the display-name
# table stays the set of the inference nodes)
