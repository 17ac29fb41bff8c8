"""Training-prep feature dump on the HIP path: mirror of the reference's `FeatureInput`
(preprocessing_utils.py:102-193).

For every sliced 16 kHz training clip it writes the HuBERT features (`3_feature768/<name>.npy`, float32 [T_h, 768] for v2 /
`3_feature256`, [T_h, 256] for v1), the coarse pitch (`2a_f0/<name>.npy`, int16 [n]) and the NSF pitch (`2b-f0nsf/<name>.npy`,
float64 [n]) - same arrays, dtypes and skip-if-present rule as the reference.  Differences: the networks are this build's HIP
graphs; `go` can shard the file list over the ranks of an initialised process group (files are independent: clip i -> rank
i mod N, no collective); audio files are read with scipy (PCM / float WAV) because soundfile / librosa / ffmpeg are not available
offline - other containers raise.  A WAV at another rate is resampled to 16 kHz on load like the reference does (preprocessing_utils.py:171 ->
load_input_audio(path, 16000) -> librosa.resample), here with the device polyphase kernel of lib/audio.py::resample_audio - PARITY-UNPINNED like the
two other resampling branches (librosa / soxr absent: the kernel is pinned to its own float64 definition, tests/test_hip_ops.py).
Note the reference's quirk that training prep quantises the pitch with f0_max = 1100 Hz (get_f0's default) while inference uses
1600 Hz (vc_infer_pipeline.py:118).
"""
import os
import sys
import traceback

import numpy as np
import torch

from .config import Config
from .lib import dataset_prep
from .lib.audio import hz_to_mel
from .lib.utils import gc_collect
from .pitch_extraction import FeatureExtractor


def load_wav(path, sr, device="cuda:0"):
    """float32 mono / stereo samples in [-1, 1) of a WAV file at the working rate `sr` (resampled on the device when the file has another rate)."""
    from scipy.io import wavfile   # noqa: PLC0415
    rate, data = wavfile.read(path)
    if data.dtype == np.int16:
        x = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        x = data.astype(np.float32) / 2147483648.0
    elif data.dtype == np.uint8:
        x = (data.astype(np.float32) - 128.0) / 128.0
    else:
        x = data.astype(np.float32)
    if rate != sr:
        from .lib.audio import resample_audio   # noqa: PLC0415
        x = resample_audio(x.T if x.ndim > 1 else x, rate, sr, device=device)       # along the last axis, like librosa.resample
        x = np.ascontiguousarray(x.T) if x.ndim > 1 else x
    return x, sr


class Preprocess:
    """Slices the recordings of a folder into training clips (mirror of the reference's `Preprocess`, preprocessing_utils.py:13-100):
    `exp_dir/0_gt_wavs/{idx0}_{idx1}.wav` at the model rate `sr` and `exp_dir/1_16k_wavs/{idx0}_{idx1}.wav` at 16 kHz, peak-limited to
    `max_volume`, both IEEE-float WAV; `exp_dir/preprocess.log` gets the same lines.  Slicer parameters, window arithmetic and file numbering are
    the reference's (lib/dataset_prep.py::plan_windows, including the numbers a remainder shares with the next chunk's first window).

    Differences: filter, RMS, cut and resampling run on the device, one launch sequence per recording (lib/dataset_prep.py); the high-pass is
    evaluated in its sections form, so samples differ from scipy's lfilter by that routine's own rounding noise; files are read with
    `load_wav` (WAV only), and a stereo file is AVERAGED TO MONO before slicing (the reference slices what its loader returns, which is mono);
    `preprocessor`, when given, is any callable (audio, sr) -> (audio, sr) applied on the host; `n_p` only partitions the file list - there is one
    process and one device, so `noparallel` is accepted and ignored."""

    def __init__(self, sr, exp_dir, preprocessor=None, noparallel=True, period=3.0, overlap=.3, max_volume=.95, device="cuda:0"):
        self.slicer = dataset_prep.slicer_params(sr)
        self.sr = sr
        self.per = period
        self.overlap = overlap
        self.tail = self.per + self.overlap
        self.max_volume = max_volume
        self.exp_dir = exp_dir
        self.gt_wavs_dir = os.path.join(exp_dir, "0_gt_wavs")
        self.wavs16k_dir = os.path.join(exp_dir, "1_16k_wavs")
        self.noparallel = noparallel
        self.preprocessor = preprocessor
        self.device = device
        os.makedirs(self.exp_dir, exist_ok=True)
        os.makedirs(self.gt_wavs_dir, exist_ok=True)
        os.makedirs(self.wavs16k_dir, exist_ok=True)

    def println(self, strr):
        print(strr)
        with open("%s/preprocess.log" % self.exp_dir, "a+") as f:
            f.write("%s\n" % strr)
            f.flush()

    def norm_write(self, tmp_audio, idx0, idx1, audio16k=None):
        """Writes one clip pair if it is longer than 2 * overlap s.  `audio16k` is the clip's peak-limited 16 kHz version when the caller already
        has it (pipeline: rvc_cut_windows); without it the clip takes the per-clip route (remix_audio), as in the reference."""
        from scipy.io import wavfile   # noqa: PLC0415
        if len(tmp_audio) > self.overlap * self.sr * 2:
            if audio16k is None:
                from .lib.audio import remix_audio   # noqa: PLC0415
                audio16k = remix_audio((tmp_audio, self.sr), target_sr=16000, max_volume=self.max_volume, device=self.device)[0]
            wavfile.write(os.path.join(self.gt_wavs_dir, f"{idx0}_{idx1}.wav"), self.sr, np.asarray(tmp_audio).astype(np.float32))
            wavfile.write(os.path.join(self.wavs16k_dir, f"{idx0}_{idx1}.wav"), 16000, np.asarray(audio16k).astype(np.float32))
        else:
            print(f"skipped short audio clip: {idx0}_{idx1}.wav ({len(tmp_audio)=})")

    def slice_on_device(self, audio):
        """float32 / float64 mono recording -> (filtered float64 CUDA tensor, window plan of lib/dataset_prep.py::plan_windows)."""
        sp = self.slicer
        x = torch.from_numpy(np.ascontiguousarray(audio)).to(self.device)
        filt = dataset_prep.lfilter_hp(x, self.sr)
        n = int(x.numel())
        tags, nf = [], 0
        if n > sp["min_length"]:              # (a sample count against a frame count: the reference's early return, kept)
            rms = dataset_prep.frame_rms(filt, sp["win_size"], sp["hop_size"]).cpu().numpy()
            nf = rms.shape[0]
            tags = dataset_prep.slice_tags(rms, n, sp)
        chunks = dataset_prep.chunk_bounds(tags, nf, sp["hop_size"], n)
        return filt, dataset_prep.plan_windows(chunks, self.sr, self.per, self.overlap)

    def pipeline(self, path, idx0):
        try:
            audio, _ = load_wav(path, self.sr, self.device)
            if audio.ndim > 1:
                audio = audio.mean(-1)                                     # [N, C] -> mono
            if self.preprocessor is not None:
                audio, _ = self.preprocessor(audio, self.sr)
                audio = np.asarray(audio)
            if audio.dtype not in (np.float32, np.float64):
                audio = audio.astype(np.float32)
            filt, plan = self.slice_on_device(audio)
            todo = [(start, length, idx1) for start, length, idx1, written in plan if written]
            gt, y16 = dataset_prep.cut_windows(filt, [(s_, l_) for s_, l_, _ in todo], self.sr, self.max_volume)
            for (start, length, idx1), a, b in zip(todo, gt, y16):
                self.norm_write(a, idx0, idx1, b)
            for start, length, idx1, written in plan:
                if not written:
                    print(f"skipped short audio clip: {idx0}_{idx1}.wav (len(tmp_audio)={length})")
            self.println("%s->Suc." % path)
        except Exception:   # noqa: BLE001 - reference behaviour: log and continue
            self.println("%s->%s" % (path, traceback.format_exc()))

    def pipeline_mp(self, infos):
        for path, idx0 in infos:
            self.pipeline(path, idx0)

    def pipeline_mp_inp_dir(self, inp_root, n_p):
        try:
            infos = [("%s/%s" % (inp_root, name), idx) for idx, name in enumerate(sorted(list(os.listdir(inp_root))))]
            n_p = max(int(n_p), 1)
            for i in range(n_p):
                self.pipeline_mp(infos[i::n_p])
        except Exception:   # noqa: BLE001 - reference behaviour
            self.println("Fail. %s" % traceback.format_exc())


class FeatureInput(FeatureExtractor):
    def __init__(self, model, f0_method, exp_dir, samplerate=16000, hop_size=160, device="cuda:0", version="v2", if_f0=False, config=None):
        self.sr = samplerate
        self.hop = hop_size
        self.f0_method = f0_method
        self.exp_dir = exp_dir
        self.version = version
        self.if_f0 = if_f0
        self.f0_bin = 256
        self.f0_max = 1100.0
        self.f0_min = 50.0
        self.f0_mel_min = hz_to_mel(self.f0_min)
        self.f0_mel_max = hz_to_mel(self.f0_max)
        self.model = model
        super().__init__(samplerate, config if config is not None else Config(device=device), onnx=False)
        self.device = device

    def printt(self, strr):
        print(strr)
        if self.exp_dir:
            with open("%s/extract_f0_feature.log" % self.exp_dir, "a+") as f:
                f.write("%s\n" % strr)
                f.flush()

    def compute_feats(self, x):
        feats = torch.from_numpy(np.asarray(x)).float()
        if feats.dim() == 2:  # double channels
            feats = feats.mean(-1)
        assert feats.dim() == 1, feats.dim()
        feats = feats.view(1, -1)
        feats = self.model.extract_features(version=self.version, source=feats, padding_mask=None,
                                            output_layer=9 if self.version == "v1" else 12)
        feats = feats.squeeze(0).float().cpu().numpy()
        if np.isnan(feats).sum() == 0:
            return feats
        return self.printt("==contains nan==")

    def compute_f0(self, x):
        return self.get_f0(x, 0, self.f0_method, crepe_hop_length=self.hop)

    def go(self, paths, shard=True):
        """paths: [(wav, coarse_f0_out, nsf_f0_out, feature_out), ...] (output paths without the .npy suffix).  With an initialised
        torch.distributed process group and shard=True every rank handles paths[rank::world]."""
        if shard and torch.distributed.is_available() and torch.distributed.is_initialized():
            paths = paths[torch.distributed.get_rank()::torch.distributed.get_world_size()]
        if len(paths) == 0:
            self.printt("no-f0-todo")
            return 0
        self.printt("todo-f0-%s" % len(paths))
        done = 0
        for idx, (inp_path, opt_path1, opt_path2, opt_path3) in enumerate(paths):
            try:
                if os.path.exists(opt_path1 + ".npy") and os.path.exists(opt_path2 + ".npy") and os.path.exists(opt_path3 + ".npy"):
                    continue
                x, _ = load_wav(inp_path, self.sr, self.device)
                if self.model:
                    feats = self.compute_feats(x)
                    if feats is not None:
                        np.save(opt_path3, feats, allow_pickle=False)          # features
                        if self.if_f0:                                           # uses pitch
                            coarse_pit, featur_pit = self.compute_f0(x if x.ndim == 1 else x.mean(-1))
                            np.save(opt_path2, featur_pit, allow_pickle=False)  # nsf
                            np.save(opt_path1, coarse_pit, allow_pickle=False)  # ori
                        done += 1
            except Exception:   # noqa: BLE001 - reference behaviour: log and continue
                self.printt("f0fail-%s-%s-%s" % (idx, inp_path, traceback.format_exc()))
        return done


def preprocess_trainset(inp_root, sr, n_p, exp_dir, preprocessor=None, period=3.0, overlap=.3, max_volume=1., device="cuda:0"):
    """Folder of recordings -> sliced training clips under exp_dir (reference preprocessing_utils.py:195-208); True / False like the reference."""
    try:
        pp = Preprocess(sr, exp_dir, preprocessor=preprocessor, period=period, overlap=overlap, max_volume=max_volume, device=device)
        pp.println("start preprocess")
        pp.println(sys.argv)
        pp.pipeline_mp_inp_dir(inp_root, n_p)
        pp.println("end preprocess")
        del pp
        gc_collect()
        print("Successfully preprocessed data")
        return True
    except Exception as e:   # noqa: BLE001 - reference behaviour
        print(f"Failed to preprocess data: {e}")
        return False


# (n_fft, hop, window) of the reference's configs/*.json by model rate: 32k.json / 32k_v2.json, 40k.json, 48k.json / 48k_v2.json
SPEC_GEOMETRY = {32000: (1024, 320, 1024), 40000: (2048, 400, 2048), 48000: (2048, 480, 2048)}


def cache_spectrograms_trainset(exp_dir, sr_or_hparams, device="cuda:0", rank=0, world=1, max_batch_bytes=256 << 20):
    """Writes `{clip}.spec.pt` next to every exp_dir/0_gt_wavs/*.wav that has none: the linear spectrogram TextAudioLoaderMultiNSFsid.get_audio would
    compute and cache on first touch (reference lib/train/data_utils.py:93-131), a CPU float32 [n_fft / 2 + 1, samples // hop] tensor saved with
    _use_new_zipfile_serialization=False as the reference saves it.  sr_or_hparams: a model rate (32000 / 40000 / 48000: the geometry of the reference's
    configs) or an object with sampling_rate, filter_length, hop_length and win_length (lib/train/utils.py::HParams, or its `data` section).  The sorted
    file list is sharded rank::world like FeatureInput.go; the clips are packed into ragged batches of at most max_batch_bytes of output and every batch
    is ONE rvc_spectrogram_batch launch.  Existing caches are left alone (the loaders would load them).  Returns the number of files written."""
    from scipy.io import wavfile   # noqa: PLC0415
    from .lib.train import mel_processing as MP   # noqa: PLC0415
    if isinstance(sr_or_hparams, (int, np.integer)):
        sr = int(sr_or_hparams)
        if sr not in SPEC_GEOMETRY:
            raise ValueError(f"no training configuration for {sr} Hz: pass hparams")
        n_fft, hop, win = SPEC_GEOMETRY[sr]
    else:
        hp = getattr(sr_or_hparams, "data", sr_or_hparams)
        sr, n_fft, hop, win = int(hp.sampling_rate), int(hp.filter_length), int(hp.hop_length), int(hp.win_length)
    gt_dir = os.path.join(exp_dir, "0_gt_wavs")
    names = sorted(n for n in os.listdir(gt_dir) if n.endswith(".wav"))[int(rank)::max(int(world), 1)]
    todo = [os.path.join(gt_dir, n) for n in names if not os.path.exists(os.path.join(gt_dir, n.replace(".wav", ".spec.pt")))]
    bins, written, i = n_fft // 2 + 1, 0, 0
    while i < len(todo):
        paths, clips, nbytes = [], [], 0
        while i < len(todo) and (not clips or nbytes < max_batch_bytes):
            rate, data = wavfile.read(todo[i])
            if rate != sr:
                raise ValueError("{} SR doesn't match target {} SR".format(rate, sr))
            x = np.asarray(data).astype(np.float32)
            paths.append(todo[i])
            clips.append(x if x.ndim == 1 else x.mean(-1))
            nbytes += bins * (-(-(x.shape[0] // hop) // MP.FRAME_ALIGN) * MP.FRAME_ALIGN) * 4
            i += 1
        packed, cols = MP.spectrogram_batch(clips, n_fft, hop, win, device=device)
        host = packed.cpu()
        for path, (col, nf) in zip(paths, cols.tolist()):
            torch.save(host[:, col:col + nf].clone(), path.replace(".wav", ".spec.pt"), _use_new_zipfile_serialization=False)
            written += 1
    return written


def extract_features_trainset(hubert_model, exp_dir, n_p, f0method, device, version, if_f0, crepe_hop_length):
    """HuBERT features and pitch of every clip in exp_dir/1_16k_wavs (reference preprocessing_utils.py:210-253): outputs named
    "{f0method},{clip}" under 2a_f0, 2b-f0nsf and 3_feature768 (3_feature256 for v1); inputs with "spec" in their path are skipped.  `n_p`
    partitions the list, every part runs on the one device in turn."""
    try:
        dev = str(device) if device is not None and str(device).startswith("cuda") else "cuda:0"
        if dev == "cuda":
            dev = "cuda:0"
        feature_input = FeatureInput(f0_method=f0method, exp_dir=exp_dir, device=dev, version=version, if_f0=if_f0, model=hubert_model,
                                     hop_size=crepe_hop_length)
        inp_root = os.path.join(exp_dir, "1_16k_wavs")
        opt_root1 = os.path.join(exp_dir, "2a_f0")
        opt_root2 = os.path.join(exp_dir, "2b-f0nsf")
        opt_root3 = os.path.join(exp_dir, "3_feature256" if version == "v1" else "3_feature768")
        for d in (opt_root1, opt_root2, opt_root3):
            os.makedirs(d, exist_ok=True)
        paths = []
        for name in sorted(list(os.listdir(inp_root))):
            inp_path = os.path.join(inp_root, name)
            if "spec" in inp_path:
                continue
            out_name = ",".join([str(f0method), name])
            paths.append([inp_path, os.path.join(opt_root1, out_name), os.path.join(opt_root2, out_name), os.path.join(opt_root3, out_name)])
        n_p = max(int(n_p), 1)
        for i in range(n_p):
            feature_input.go(paths[i::n_p])
        print(f"Successfully extracted features using {f0method}")
        return True
    except Exception as e:   # noqa: BLE001 - reference behaviour
        print(f"Failed to extract features: {e}")
        return False
