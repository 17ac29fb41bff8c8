"""Training batch loaders (mirror of the reference's lib/train/data_utils.py): datasets over a filelist.txt, their collates, and the bucket samplers.

Constructor arguments, item tuples, collate outputs and sampler batches are the reference's (tests/golden/train_loader_cases.npz holds what the
reference makes of a synthetic file list).  The one difference: a missing `{clip}.spec.pt` is computed by the device spectrogram
(mel_processing.spectrogram_torch on `spec_device`, default cuda:0) instead of torch.stft on the host, then written the way the reference writes it.
With the cache already filled (preprocessing_utils.cache_spectrograms_trainset) the loaders never touch the device, so DataLoader workers are safe.

Three quirks of the reference are kept on purpose:
  * the bucketing length of a clip is os.path.getsize(wav) // (3 * hop_length) - the file size in BYTES over three hops, not its frame count
    (a float32 WAV has 4 bytes per sample, so this is ~4/3 of the frames; bucket boundaries are chosen against these numbers);
  * labels (phone, pitch, pitchf) are cut at 900 frames whatever the clip's length;
  * an empty bucket is removed TOGETHER WITH ITS UPPER BOUNDARY (boundaries.pop(i + 1), on the caller's list), so the bucket below it widens.
"""
import os
import traceback

import numpy as np
import torch
import torch.utils.data

from .mel_processing import spectrogram_torch
from .utils import load_filepaths_and_text, load_wav_to_torch

MAX_LABEL_FRAMES = 900


class _ClipDataset(torch.utils.data.Dataset):
    """What the two datasets share: hyper-parameters, the length filter, the cached spectrogram."""
    n_fields = 0                 # columns of a file-list row
    spec_device = "cuda:0"       # where a missing spectrogram is computed

    def __init__(self, audiopaths_and_text, hparams):
        self.audiopaths_and_text = load_filepaths_and_text(audiopaths_and_text)
        self.max_wav_value = hparams.max_wav_value
        self.sampling_rate = hparams.sampling_rate
        self.filter_length = hparams.filter_length
        self.hop_length = hparams.hop_length
        self.win_length = hparams.win_length
        self.min_text_len = getattr(hparams, "min_text_len", 1)
        self.max_text_len = getattr(hparams, "max_text_len", 5000)
        self._filter()

    def _filter(self):
        """Keeps the rows whose text field (a path: its LENGTH IN CHARACTERS is what is compared) lies in [min_text_len, max_text_len] and stores the
        bucketing lengths - quirk 1 of the module docstring."""
        rows, lengths = [], []
        for row in self.audiopaths_and_text:
            row = list(row[:self.n_fields]) if len(row) == self.n_fields else self._bad_row(row)
            if self.min_text_len <= len(row[1]) <= self.max_text_len:
                rows.append(row)
                lengths.append(os.path.getsize(row[0]) // (3 * self.hop_length))
        self.audiopaths_and_text = rows
        self.lengths = lengths

    def _bad_row(self, row):
        raise ValueError(f"a file-list row has {len(row)} fields, expected {self.n_fields}: {row}")

    def get_sid(self, sid):
        return torch.LongTensor([int(sid)])

    def _compute_spec(self, audio_norm, spec_filename):
        spec = spectrogram_torch(audio_norm.to(self.spec_device), self.filter_length, self.hop_length, self.win_length, center=False)
        spec = torch.squeeze(spec, 0).cpu()
        torch.save(spec, spec_filename, _use_new_zipfile_serialization=False)
        return spec

    def get_audio(self, filename):
        """(spec [n_fft / 2 + 1, frames], wav [1, samples]) of a clip; the spectrogram from `{clip}.spec.pt` when that loads, else computed and cached."""
        audio, sampling_rate = load_wav_to_torch(filename)
        if sampling_rate != self.sampling_rate:
            raise ValueError("{} SR doesn't match target {} SR".format(sampling_rate, self.sampling_rate))
        audio_norm = audio.unsqueeze(0)
        spec_filename = filename.replace(".wav", ".spec.pt")
        if os.path.exists(spec_filename):
            try:
                return torch.load(spec_filename), audio_norm
            except Exception:   # noqa: BLE001 - reference behaviour: report, recompute, overwrite
                print(spec_filename, traceback.format_exc())
        return self._compute_spec(audio_norm, spec_filename), audio_norm

    def __getitem__(self, index):
        return self.get_audio_text_pair(self.audiopaths_and_text[index])

    def __len__(self):
        return len(self.audiopaths_and_text)


def _load_phone(path):
    phone = np.repeat(np.load(path), 2, axis=0)          # 50 fps features -> 100 fps
    return phone[:min(phone.shape[0], MAX_LABEL_FRAMES), :]      # quirk 2


class TextAudioLoaderMultiNSFsid(_ClipDataset):
    """Rows `wav|phone.npy|pitch.npy|pitchf.npy|speaker` -> (spec, wav, phone, pitch, pitchf, sid), all cut to the shorter of the label and the
    spectrogram lengths (wav to that many hops)."""
    n_fields = 5

    def get_labels(self, phone, pitch, pitchf):
        phone = _load_phone(phone)
        n = phone.shape[0]
        pitch = np.load(pitch)[:n]
        pitchf = np.load(pitchf)[:n]
        return torch.FloatTensor(phone), torch.LongTensor(pitch), torch.FloatTensor(pitchf)

    def get_audio_text_pair(self, audiopath_and_text):
        file, phone, pitch, pitchf, dv = audiopath_and_text
        phone, pitch, pitchf = self.get_labels(phone, pitch, pitchf)
        spec, wav = self.get_audio(file)
        dv = self.get_sid(dv)
        len_phone, len_spec = phone.size(0), spec.size(-1)
        if len_phone != len_spec:
            n = min(len_phone, len_spec)
            spec, wav = spec[:, :n], wav[:, :n * self.hop_length]
            phone, pitch, pitchf = phone[:n, :], pitch[:n], pitchf[:n]
        return (spec, wav, phone, pitch, pitchf, dv)


class TextAudioLoader(_ClipDataset):
    """Rows `wav|phone.npy|speaker` (models without pitch) -> (spec, wav, phone, sid)."""
    n_fields = 3

    def get_labels(self, phone):
        return torch.FloatTensor(_load_phone(phone))

    def get_audio_text_pair(self, audiopath_and_text):
        file, phone, dv = audiopath_and_text
        phone = self.get_labels(phone)
        spec, wav = self.get_audio(file)
        dv = self.get_sid(dv)
        len_phone, len_spec = phone.size(0), spec.size(-1)
        if len_phone != len_spec:
            n = min(len_phone, len_spec)
            spec, wav, phone = spec[:, :n], wav[:, :n * self.hop_length], phone[:n, :]
        return (spec, wav, phone, dv)


def _collate(batch, with_pitch):
    """Zero-pads a list of dataset items to the batch's longest, rows ordered by spectrogram length, longest first (torch.sort's order among equals)."""
    n = len(batch)
    _, order = torch.sort(torch.LongTensor([x[0].size(1) for x in batch]), dim=0, descending=True)
    spec_padded = torch.zeros(n, batch[0][0].size(0), max(x[0].size(1) for x in batch))
    wave_padded = torch.zeros(n, 1, max(x[1].size(1) for x in batch))
    max_phone = max(x[2].size(0) for x in batch)
    phone_padded = torch.zeros(n, max_phone, batch[0][2].shape[1])
    pitch_padded = torch.zeros(n, max_phone, dtype=torch.long)
    pitchf_padded = torch.zeros(n, max_phone)
    spec_lengths, wave_lengths, phone_lengths, sid = (torch.zeros(n, dtype=torch.long) for _ in range(4))
    for i, src in enumerate(order.tolist()):
        row = batch[src]
        spec, wave, phone = row[0], row[1], row[2]
        spec_padded[i, :, :spec.size(1)] = spec
        spec_lengths[i] = spec.size(1)
        wave_padded[i, :, :wave.size(1)] = wave
        wave_lengths[i] = wave.size(1)
        phone_padded[i, :phone.size(0), :] = phone
        phone_lengths[i] = phone.size(0)
        if with_pitch:
            pitch_padded[i, :row[3].size(0)] = row[3]
            pitchf_padded[i, :row[4].size(0)] = row[4]
        sid[i] = row[-1]
    if with_pitch:
        return (phone_padded, phone_lengths, pitch_padded, pitchf_padded, spec_padded, spec_lengths, wave_padded, wave_lengths, sid)
    return (phone_padded, phone_lengths, spec_padded, spec_lengths, wave_padded, wave_lengths, sid)


class TextAudioCollateMultiNSFsid:
    """Items of TextAudioLoaderMultiNSFsid -> (phone, phone_lengths, pitch, pitchf, spec, spec_lengths, wave, wave_lengths, sid)."""

    def __init__(self, return_ids=False):
        self.return_ids = return_ids

    def __call__(self, batch):
        return _collate(batch, True)


class TextAudioCollate:
    """Items of TextAudioLoader -> (phone, phone_lengths, spec, spec_lengths, wave, wave_lengths, sid)."""

    def __init__(self, return_ids=False):
        self.return_ids = return_ids

    def __call__(self, batch):
        return _collate(batch, False)


class _Buckets:
    """Length buckets (b[i], b[i + 1]] over dataset.lengths; clips outside (b[0], b[-1]] are dropped.  `group` = samples per step over all replicas:
    every bucket is filled up to a multiple of it by repeating its own members."""

    def _create_buckets(self, group):
        buckets = [[] for _ in range(len(self.boundaries) - 1)]
        for i, length in enumerate(self.lengths):
            b = self._bisect(length)
            if b != -1:
                buckets[b].append(i)
        for i in range(len(buckets) - 1, -1, -1):
            if not buckets[i]:
                buckets.pop(i)
                self.boundaries.pop(i + 1)                     # quirk 3: the caller's list loses the EMPTY bucket's upper boundary
        return buckets, [len(b) + (group - len(b) % group) % group for b in buckets]

    def _bisect(self, x, lo=0, hi=None):
        if hi is None:
            hi = len(self.boundaries) - 1
        while hi > lo:
            mid = (hi + lo) // 2
            if self.boundaries[mid] < x <= self.boundaries[mid + 1]:
                return mid
            if x <= self.boundaries[mid]:
                hi = mid
            else:
                lo = mid + 1
        return -1

    def _batches(self, rank, replicas):
        """The epoch's batches of this rank: per bucket a permutation (seeded by the epoch), filled up by repetition, every replicas-th member from
        `rank`, cut into batches; then the batches themselves permuted."""
        g = torch.Generator()
        g.manual_seed(self.epoch)
        if self.shuffle:
            orders = [torch.randperm(len(b), generator=g).tolist() for b in self.buckets]
        else:
            orders = [list(range(len(b))) for b in self.buckets]
        batches = []
        for bucket, ids, total in zip(self.buckets, orders, self.num_samples_per_bucket):
            rem = total - len(bucket)
            ids = ids + ids * (rem // len(bucket)) + ids[:rem % len(bucket)]
            ids = ids[rank::replicas]
            for j in range(len(ids) // self.batch_size):
                batches.append([bucket[k] for k in ids[j * self.batch_size:(j + 1) * self.batch_size]])
        if self.shuffle:
            batches = [batches[i] for i in torch.randperm(len(batches), generator=g).tolist()]
        return batches


class DistributedBucketSampler(_Buckets, torch.utils.data.distributed.DistributedSampler):
    """Batches of similar length for one rank of a data-parallel run; the replicas' batches of an epoch partition the (filled-up) buckets."""

    def __init__(self, dataset, batch_size, boundaries, num_replicas=None, rank=None, shuffle=True):
        torch.utils.data.distributed.DistributedSampler.__init__(self, dataset, num_replicas=num_replicas, rank=rank, shuffle=shuffle)
        self.lengths = dataset.lengths
        self.batch_size = batch_size
        self.boundaries = boundaries
        self.buckets, self.num_samples_per_bucket = self._create_buckets(self.num_replicas * self.batch_size)
        self.total_size = sum(self.num_samples_per_bucket)
        self.num_samples = self.total_size // self.num_replicas

    def __iter__(self):
        self.batches = self._batches(self.rank, self.num_replicas)
        assert len(self.batches) * self.batch_size == self.num_samples
        return iter(self.batches)

    def __len__(self):
        return self.num_samples // self.batch_size


class BucketSampler(_Buckets, torch.utils.data.Sampler):
    """The single-process sampler: the same buckets and batches as DistributedBucketSampler with one replica."""

    def __init__(self, dataset, batch_size, boundaries, shuffle=True):
        self.lengths = dataset.lengths
        self.batch_size = batch_size
        self.boundaries = boundaries
        self.shuffle = shuffle
        self.epoch = 0
        self.buckets, self.num_samples_per_bucket = self._create_buckets(self.batch_size)
        self.total_size = sum(self.num_samples_per_bucket)

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __iter__(self):
        self.batches = self._batches(0, 1)
        return iter(self.batches)

    def __len__(self):
        return self.total_size // self.batch_size
