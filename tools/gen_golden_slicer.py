"""Writes tests/golden/slicer_cases.npz: what the REFERENCE's slicer and Preprocess make of the recordings of synthetic.slicer_test_signal.

Build container only (needs the reference tree, RVC_REFERENCE_ROOT; no test and no GPU job runs this).  The reference's lib/slicer2.py is loaded
by path at run time and its Preprocess through oracle/ref_shim.py, with the file reader, the WAV writer and the resampler of that module replaced
by recorders - only the slicing and the window / name arithmetic run.  Per case the file holds arrays and names, no audio:
  {case}_rms        float64 [n_frames]   the RMS list Slicer.slice scanned (of ITS lfilter output)
  {case}_tags       int64 [n_tags][2]    sil_tags
  {case}_argmin     int64 [n][2]         every [a, b) range the scan took an arg-min over (clipped to the list)
  {case}_chunks     int64 [n_chunks][2]  (begin, end) of every chunk in samples
  {case}_windows    int64 [n_win][4]     (start, length, idx1, written) in the order Preprocess.pipeline reaches norm_write
  {case}_names      str [n_files]        sorted names "{idx0}_{idx1}" left in 0_gt_wavs (a later window overwrites an earlier one of the same name)
  {case}_meta       int64 [4]            sr, seed, idx0, n_samples
Every case must be well-posed for an equality check (asserted here and again by the tests on these values): no RMS frame within 1 % of the
threshold, and in every arg-min range the two smallest values differ by more than 1e-3 relative.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from comfy_rvc_amd import synthetic as S   # noqa: E402

REF_ROOT = os.environ.get("RVC_REFERENCE_ROOT", "/root/reference")
# name -> (sr, seed, segments, idx0)
CASES = {
    "r40k_s0": (40000, 0, S.SLICER_SEGMENTS, 0),
    "short_sil_40k": (40000, 0, S.SLICER_SEGMENTS_SHORT_SIL, 1),
    "r48k_s0": (48000, 0, S.SLICER_SEGMENTS, 0),
    "r32k_s1": (32000, 1, S.SLICER_SEGMENTS, 0),
    "tiny_40k": (40000, 3, (("v", 0.0025),), 0),          # 100 samples = min_length frames: the early return
}


class _Rec(np.ndarray):
    """The RMS list as the scan sees it; remembers the slice an arg-min is taken over."""
    log = None

    def __getitem__(self, k):
        r = super().__getitem__(k)
        if isinstance(k, slice) and isinstance(r, _Rec):
            n = self.shape[0]
            r._range = k.indices(n)[:2]
        return r

    def argmin(self, *a, **k):
        _Rec.log.append(tuple(int(v) for v in self._range))
        return np.asarray(self).argmin(*a, **k)


def well_posed(rms, threshold, ranges):
    if rms.size and np.abs(rms / threshold - 1.0).min() <= 0.01:
        return False
    for a, b in ranges:
        v = np.sort(rms[a:b])
        if v.size > 1 and (v[1] - v[0]) <= 1e-3 * v[0]:
            return False
    return True


def main():
    spec = importlib.util.spec_from_file_location("ref_slicer2", os.path.join(REF_ROOT, "lib", "slicer2.py"))
    slicer2 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(slicer2)
    from oracle import ref_shim
    pu = ref_shim.load_preprocessing_utils()
    import tempfile
    out = {}
    for case, (sr, seed, segments, idx0) in CASES.items():
        x = S.slicer_test_signal(sr, seed, segments)
        state = {"rms": np.zeros(0), "windows": [], "written": [], "tags": []}
        orig_rms = slicer2.get_rms

        def get_rms(**kw):
            r = orig_rms(**kw)
            state["rms"] = np.array(r).reshape(-1)
            return r.view(_Rec)

        _Rec.log = []

        class Wav:
            @staticmethod
            def write(path, rate, data):
                state["written"].append((os.path.basename(os.path.dirname(path)), os.path.basename(path), int(rate), int(len(data))))

        class P(pu.Preprocess):
            def norm_write(self, tmp_audio, idx0_, idx1):
                base = tmp_audio.base if tmp_audio.base is not None else tmp_audio
                start = (tmp_audio.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // tmp_audio.itemsize if len(tmp_audio) else -1
                before = len(state["written"])
                super().norm_write(tmp_audio, idx0_, idx1)
                state["windows"].append((int(start), int(len(tmp_audio)), int(idx1), int(len(state["written"]) > before)))

        with tempfile.TemporaryDirectory() as tmp:
            pp = P(sr, tmp)
            # the slicer of the module loaded by path, same parameters as Preprocess.__init__ passes
            ref = pp.slicer
            sl = slicer2.Slicer(sr=sr, threshold=-50, min_length=1500, min_interval=400, hop_size=15, max_sil_kept=500)
            assert (sl.threshold, sl.hop_size, sl.win_size, sl.min_length, sl.min_interval, sl.max_sil_kept) == \
                (ref.threshold, ref.hop_size, ref.win_size, ref.min_length, ref.min_interval, ref.max_sil_kept)
            pp.slicer = sl
            chunks = []
            orig_slice = sl.slice

            def slice_(waveform):
                res = orig_slice(waveform)
                for c in res:
                    base = c.base if c.base is not None else c
                    b = (c.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // c.itemsize
                    chunks.append((int(b), int(b + len(c))))
                return res

            sl.slice = slice_
            slicer2.get_rms = get_rms
            saved = pu.load_input_audio, pu.wavfile, pu.remix_audio
            pu.load_input_audio = lambda path, sr_: (x, sr_)
            pu.wavfile = Wav
            pu.remix_audio = lambda a, target_sr=None, **k: (np.zeros(1, dtype=np.float32), target_sr)
            def profile(frame, event, arg):      # sil_tags is a local of Slicer.slice: read when that frame returns
                if event == "return" and frame.f_code is slicer2.Slicer.slice.__code__:
                    state["tags"] = [(int(b), int(e)) for b, e in frame.f_locals.get("sil_tags", [])]

            sys.setprofile(profile)
            try:
                pp.pipeline("case.wav", idx0)
            finally:
                sys.setprofile(None)
                slicer2.get_rms = orig_rms
                pu.load_input_audio, pu.wavfile, pu.remix_audio = saved
            log = open(os.path.join(tmp, "preprocess.log")).read()
            assert "->Suc." in log, log
        rms = state["rms"]
        tags = state["tags"]
        assert well_posed(rms, sl.threshold, _Rec.log), f"{case}: not well-posed for an equality check - choose another seed"
        names = sorted(set(n for d, n, r, ln in state["written"] if d == "0_gt_wavs"))
        out[f"{case}_rms"] = rms
        out[f"{case}_tags"] = np.array(tags, dtype=np.int64).reshape(-1, 2)
        out[f"{case}_argmin"] = np.array(_Rec.log, dtype=np.int64).reshape(-1, 2)
        out[f"{case}_chunks"] = np.array(chunks, dtype=np.int64).reshape(-1, 2)
        out[f"{case}_windows"] = np.array(state["windows"], dtype=np.int64).reshape(-1, 4)
        out[f"{case}_names"] = np.array([n[:-4] for n in names])
        out[f"{case}_meta"] = np.array([sr, seed, idx0, len(x)], dtype=np.int64)
        print(case, "frames", rms.size, "tags", tags, "chunks", [e - b for b, e in chunks], "windows", state["windows"], "names", names)
    path = os.path.join(ROOT, "tests", "golden", "slicer_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
