"""Do two builds of the library compute the same bits?  For host-side refactors of the model graphs.
    RVC_HIP_LIB=<library> python tools/graph_biteq.py out.json        (once per library, then compare the "sha256" maps of the two files)
Runs a fixed set of cases through the loaded library - every model graph at the default precision, the four that have a plain fp32 graph once more built
at rvc_set_conv_precision(0) - and writes the SHA-256 of every tap and output, plus rvc_ctx_workspace_bytes after each case."""
import hashlib, json, os, sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from comfy_rvc_amd import _lib as L                      # noqa: E402
from comfy_rvc_amd import synthetic as S                 # noqa: E402
from comfy_rvc_amd.lib.infer_pack import models as M     # noqa: E402

SHA, WORKSPACE = {}, {}
SYNTH_TAPS = ("enc_p_layer0", "m_p", "logs_p", "z_p", "z", "har_source", "sine_waves")
FWD_TAPS = ("z", "z_p", "m_p", "logs_p", "m_q", "logs_q")


def golden(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", name)))


def put(case, name, x):
    torch.cuda.synchronize()
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    SHA[f"{case}.{name}"] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def done(case):
    WORKSPACE[case] = int(L.lib.rvc_ctx_workspace_bytes(L.get_ctx(0)))


def hubert_case(case):
    from comfy_rvc_amd.lib.infer_pack.loaders import HubertModelWithFinalProj
    hub = HubertModelWithFinalProj(S.hubert_state_dict(0), S.HUBERT_CONFIG)
    audio = torch.from_numpy(golden("hubert_1s.npz")["audio"])
    Th = hub.num_frames(audio.shape[1])
    taps = {"conv_stack": torch.empty(512, Th, device="cuda"), "pos_conv": torch.empty(768, Th, device="cuda"),
            "hidden_0": torch.empty(768, Th, device="cuda"), "hidden_8": torch.empty(768, Th, device="cuda")}
    put(case, "v2", hub.extract_features(audio, version="v2", taps=taps))
    for k, v in taps.items():
        put(case, k, v)
    put(case, "v1", hub.extract_features(audio, version="v1"))
    done(case)


def rmvpe_case(case):
    from comfy_rvc_amd.lib.rmvpe import RMVPE
    net = RMVPE(S.rmvpe_state_dict(0), is_half=False)
    g = golden("rmvpe_1s.npz")
    r = net.infer(g["audio"], want_mel=True, want_salience=True)
    for k in ("mel", "salience", "f0"):
        put(case, k, r[k])
    put(case, "decode", net.decode(g["syn_salience"]))
    done(case)


def synth_net(f0=True):
    net = M.SynthesizerTrnMs768NSFsid(*S.CONFIG_40K_V2, is_half=False) if f0 else M.SynthesizerTrnMs768NSFsid_nono(*S.CONFIG_40K_V2)
    return net.load_state_dict(S.synth_state_dict(S.CONFIG_40K_V2, "v2", 0, f0=f0))


def synth_golden_case(case, net, arith=None):
    g = golden("synth_40k_v2.npz")
    T = g["phone"].shape[1]
    prev = L.lib.rvc_get_pair_arithmetic()
    if arith is not None:
        L.check(L.lib.rvc_set_pair_arithmetic(arith))
    try:
        taps = {k: None for k in SYNTH_TAPS}
        o, _, _ = net.infer(torch.from_numpy(g["phone"]), torch.LongTensor([T]), torch.from_numpy(g["pitch"]), torch.from_numpy(g["pitchf"]),
                            torch.LongTensor([int(g["sid"])]), noise=(g["noise_z"], g["noise_src"]), taps=taps)
    finally:
        L.check(L.lib.rvc_set_pair_arithmetic(prev))
    put(case, "wav", o)
    for k, v in taps.items():
        put(case, k, v)
    done(case)


def synth_nono_case(case):
    net = synth_net(f0=False)
    g = golden("synth_40k_v2_nono.npz")
    T = g["phone"].shape[1]
    taps = {k: None for k in ("m_p", "logs_p", "z_p", "z")}
    o, _, _ = net.infer(torch.from_numpy(g["phone"]), torch.LongTensor([T]), torch.LongTensor([int(g["sid"])]), noise=g["noise_z"], taps=taps)
    put(case, "wav", o)
    for k, v in taps.items():
        put(case, k, v)
    done(case)


def synth_600_case(case, net):
    """600 frames of seeded inputs: the whole sequence, then the keep window [150, 450) (only the window's samples are defined and hashed)."""
    T, upp = 600, 400
    rng = np.random.default_rng(1600)
    gen = torch.Generator().manual_seed(T)
    phone = torch.from_numpy((rng.standard_normal((1, T, 768)) * 0.5).astype(np.float32))
    pitch = torch.from_numpy(rng.integers(1, 256, (1, T)).astype(np.int64))
    pitchf = torch.from_numpy(S.designed_f0(T, seed=0).astype(np.float32))[None]
    noise = (torch.randn(1, 192, T, generator=gen), torch.randn(1, T * upp, 1, generator=gen))
    a = (phone, torch.LongTensor([T]), pitch, pitchf, torch.LongTensor([0]))
    put(case, "whole", net.infer(*a, noise=noise)[0])
    put(case, "keep_150_450", net.infer(*a, noise=noise, keep=(150, 450))[0][..., 150 * upp:450 * upp])
    done(case)


def train_forward_case(case):
    g = golden("train_forward_40k_v2.npz")
    config = S.CONFIG_40K_V2
    net = M.SynthesizerTrnMs768NSFsid(*config, is_half=False)
    net.load_state_dict(S.synth_train_state_dict(config, "v2", int(g["weight_seed"]), f0=True))
    b = S.synth_train_batch(config, "v2", [int(x) for x in g["lengths"]], int(g["input_seed"]), f0=True)
    gen = torch.Generator().manual_seed(int(g["noise_seed"]))
    draws = [torch.randn(tuple(int(v) for v in s), generator=gen) for s in g["draw_shapes"]]
    t = {k: torch.from_numpy(np.asarray(v)) for k, v in b.items()}
    o, _, _, _, taps = net(t["phone"], t["lengths"], t["pitch"], t["pitchf"], t["spec"], t["lengths"], t["sid"], noise=(draws[0], draws[1]),
                           ids_slice=torch.from_numpy(g["ids_slice"]))
    put(case, "o", o)
    for k, v in zip(FWD_TAPS, taps):
        put(case, k, v)
    done(case)


def mdx23_case(case):
    from comfy_rvc_amd.lib.karafan.inference import demix_mdxv3
    from comfy_rvc_amd.lib.karafan.tfc_tdf import TFC_TDF_net
    cfg = S.mdx23c_config(**S.MDX23C_SMALL)
    net = TFC_TDF_net(cfg)
    net.load_state_dict(S.mdx23c_state_dict(cfg, 0))
    g = golden("mdx23c_small.npz")
    put(case, "chunk", net(g["x"][None])[0])
    est = demix_mdxv3(g["clip"], net, net.device, cfg, int(g["overlap"]))
    for k in sorted(est):
        put(case, "demix_" + k, est[k])
    done(case)


def crepe_case(case):
    from comfy_rvc_amd.lib.crepe import Crepe
    net = Crepe(S.crepe_state_dict("full", 0), "full")
    x = torch.from_numpy(S.synth_audio(1.3, seed=11)).to(net.device, torch.float32).contiguous()
    put(case, "probabilities", net.probabilities(x, 160, pad=True))
    done(case)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "graph_biteq.json"
    hubert_case("hubert_1s")
    rmvpe_case("rmvpe_1s")
    net = synth_net()
    synth_golden_case("synth_40k_v2.fp16x2_pairs", net, 1)
    synth_golden_case("synth_40k_v2.bf16x3_pairs", net, 0)
    synth_nono_case("synth_40k_v2_nono")
    synth_600_case("synth_600_frames", net)
    train_forward_case("train_forward_40k_v2")
    mdx23_case("mdx23c_small")
    crepe_case("crepe_full_1.3s")
    L.check(L.lib.rvc_set_conv_precision(0))      # models built from here on take the plain fp32 graph
    try:
        hubert_case("precision0.hubert_1s")
        rmvpe_case("precision0.rmvpe_1s")
        synth_golden_case("precision0.synth_40k_v2", synth_net())
        train_forward_case("precision0.train_forward_40k_v2")
    finally:
        L.check(L.lib.rvc_set_conv_precision(1))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"library": os.path.basename(L.LIB_PATH), "sha256": SHA, "workspace_bytes": WORKSPACE}, f, indent=1, sort_keys=True)
    print(f"{len(SHA)} hashes of {len(WORKSPACE)} cases -> {out}")


if __name__ == "__main__":
    main()
