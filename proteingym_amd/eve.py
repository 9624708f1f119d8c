"""EVE / DeepSequence evolutionary indices on the HIP path (``proteingym/baselines/EVE``; C ABI: the EVE section of include/pgmi.h).

Host side only: the checkpoint loader (``torch.load`` -> ``model_state_dict`` + the parameter JSON -> the fp32 blob in
``state_dict()`` order), the focus-column alignment and residue-number map of ``utils/data_utils.py`` (``MSA_processing.gen_alignment``
and ``create_all_singles``, on ``alignment.FocusAlignment``), the mutant validity rules of ``VAE_model.py:408-450`` and the ctypes
handle.  The estimator and its divergences from the reference are in DESIGN.md 4.6f.
"""
from __future__ import annotations

import ctypes as C
import json
from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import _lib
from .alignment import AMINO_ACIDS, FocusAlignment

MAX_LAYERS = 8
ACTS = {"relu": 0, "tanh": 1, "sigmoid": 2, "elu": 3, "linear": 4}
NO_LETTER = 255


class EveConfig(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("seq_len", C.c_int32), ("alphabet", C.c_int32), ("z_dim", C.c_int32),
                ("n_enc", C.c_int32), ("enc_sizes", C.c_int32 * MAX_LAYERS), ("n_dec", C.c_int32), ("dec_sizes", C.c_int32 * MAX_LAYERS),
                ("conv_depth", C.c_int32), ("temperature", C.c_int32), ("sparsity_tiles", C.c_int32),
                ("enc_act", C.c_int32), ("dec_first_act", C.c_int32), ("dec_last_act", C.c_int32), ("precision", C.c_int32),
                ("dropout_p", C.c_float)]


class EveNoise(C.Structure):
    _fields_ = [("z_eps", C.c_void_p), ("keep", C.c_void_p * (MAX_LAYERS + 1)), ("w_eps", C.c_void_p * MAX_LAYERS),
                ("b_eps", C.c_void_p * MAX_LAYERS), ("wout_eps", C.c_void_p), ("bout_eps", C.c_void_p), ("conv_eps", C.c_void_p),
                ("sparsity_eps", C.c_void_p), ("temp_eps", C.c_void_p)]


def dims_from_params(params: dict, seq_len: int) -> dict:
    """The fields of pgmi_eve_config from a parameter JSON (default_model_params.json / deepseq_model_params.json)."""
    enc, dec = params["encoder_parameters"], params["decoder_parameters"]
    if enc.get("convolve_input") or float(enc.get("dropout_proba", 0.0)) != 0.0:
        raise ValueError("EVE encoder with an input convolution or dropout is not supported (neither parameter file uses them)")
    if not dec.get("bayesian_decoder", True):
        raise ValueError("only the Bayesian decoder is supported (bayesian_decoder: true in both parameter files)")
    if int(enc["z_dim"]) != int(dec["z_dim"]):
        raise ValueError("encoder and decoder z_dim differ")
    return dict(seq_len=int(seq_len), z_dim=int(dec["z_dim"]), enc_sizes=[int(x) for x in enc["hidden_layers_sizes"]],
                dec_sizes=[int(x) for x in dec["hidden_layers_sizes"]],
                conv_depth=int(dec["convolution_output_depth"]) if dec["convolve_output"] else 0,
                temperature=int(bool(dec["include_temperature_scaler"])),
                sparsity_tiles=int(dec["num_tiles_sparsity"]) if dec["include_sparsity"] else 0,
                enc_act=enc["nonlinear_activation"], dec_first_act=dec["first_hidden_nonlinearity"],
                dec_last_act=dec["last_hidden_nonlinearity"], dropout_p=float(dec["dropout_proba"]))


def key_shapes(d: dict) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of every tensor of the blob, in VAE_model.state_dict() order (include/pgmi.h lists the same)."""
    L, z, H = d["seq_len"], d["z_dim"], d["dec_sizes"][-1]
    Cc = d["conv_depth"] or 20
    out, fan = [], 20 * L
    for i, e in enumerate(d["enc_sizes"]):
        out += [(f"encoder.hidden_layers.{i}.weight", (e, fan)), (f"encoder.hidden_layers.{i}.bias", (e,))]
        fan = e
    for n in ("fc_mean", "fc_log_var"):
        out += [(f"encoder.{n}.weight", (z, fan)), (f"encoder.{n}.bias", (z,))]
    if d["sparsity_tiles"]:
        out += [(f"decoder.sparsity_weight_{s}", (H // d["sparsity_tiles"], L)) for s in ("mean", "log_var")]
    out += [(f"decoder.last_hidden_layer_weight_{s}", (Cc * L, H)) for s in ("mean", "log_var")]
    out += [(f"decoder.last_hidden_layer_bias_{s}", (20 * L,)) for s in ("mean", "log_var")]
    if d["temperature"]:
        out += [(f"decoder.temperature_scaler_{s}", (1,)) for s in ("mean", "log_var")]
    for s in ("mean", "log_var"):
        fan = z
        for i, h in enumerate(d["dec_sizes"]):
            out += [(f"decoder.hidden_layers_{s}.{i}.weight", (h, fan)), (f"decoder.hidden_layers_{s}.{i}.bias", (h,))]
            fan = h
    if d["conv_depth"]:
        out += [(f"decoder.output_convolution_{s}.weight", (20, Cc, 1)) for s in ("mean", "log_var")]
    return out


def blob_from_state_dict(state: Dict[str, np.ndarray], d: dict) -> np.ndarray:
    """fp32 blob in key_shapes order; a missing, extra or mis-shaped tensor is a ValueError."""
    want = key_shapes(d)
    extra = set(state) - {k for k, _ in want}
    if extra:
        raise ValueError(f"checkpoint has tensors the configuration does not: {sorted(extra)}")
    parts = []
    for k, shape in want:
        if k not in state:
            raise ValueError(f"checkpoint lacks {k}")
        a = np.asarray(state[k], dtype=np.float32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{k}: shape {tuple(a.shape)}, configuration needs {tuple(shape)}")
        parts.append(a.reshape(-1))
    return np.concatenate(parts)


def state_from_blob(d: dict, blob: np.ndarray) -> Dict[str, np.ndarray]:
    """The inverse of blob_from_state_dict: name -> array views of the blob."""
    off, state = 0, {}
    for k, shape in key_shapes(d):
        n = int(np.prod(shape))
        state[k] = blob[off:off + n].reshape(shape)
        off += n
    return state


def load_checkpoint(path: str, params: dict, seq_len: int) -> Tuple[dict, np.ndarray]:
    """(dims, blob) of a reference checkpoint (``torch.save({'model_state_dict': ...})``, VAE_model.py:357-364)."""
    import torch
    ck = torch.load(path, map_location="cpu", weights_only=False)
    state = {k: v.detach().cpu().numpy() for k, v in ck["model_state_dict"].items()}
    d = dims_from_params(params, seq_len)
    return d, blob_from_state_dict(state, d)


class EveAlignment:
    """What compute_evol_indices_DMS.py reads off ``MSA_processing``: the focus sequence over the focus columns and the maps from
    residue numbers (the focus header's ``/start-stop``) to wild-type letters and focus indices."""

    def __init__(self, path: str, threshold_focus_cols_frac_gaps: float = 0.3, threshold_sequence_frac_gaps: float = 0.5):
        fa = FocusAlignment(path, preprocess=True, max_seq_gaps=threshold_sequence_frac_gaps, max_col_gaps=threshold_focus_cols_frac_gaps,
                            drop_indeterminate=True)
        self.focus_seq = fa.focus_seq
        self.focus_cols = [int(i) for i in fa.focus_cols]
        self.focus_seq_trimmed = "".join(self.focus_seq[i] for i in self.focus_cols)
        self.seq_len = len(self.focus_cols)
        start = int(fa.focus_name.split("/")[-1].split("-")[0])
        self.focus_start_loc = start
        self.uniprot_focus_col_to_wt_aa_dict = {i + start: self.focus_seq[i] for i in self.focus_cols}
        # create_all_singles: the focus index counts the letters of the 20-letter alphabet before the position
        self.pos_to_letter_idx: Dict[int, Tuple[str, int]] = {}
        idx = 0
        for i, letter in enumerate(self.focus_seq):
            if letter in AMINO_ACIDS:
                self.pos_to_letter_idx[start + i] = (letter, idx)
                idx += 1

    def in_singles(self, mut: str) -> bool:
        """``mut in mutant_to_letter_pos_idx_focus_list``: letter + position + another letter of the alphabet, as written."""
        if len(mut) < 3 or mut[-1] not in AMINO_ACIDS:
            return False
        body = mut[1:-1]
        if not body.isdigit() or str(int(body)) != body:
            return False
        hit = self.pos_to_letter_idx.get(int(body))
        return hit is not None and hit[0] == mut[0] and mut[-1] != mut[0]


def valid_mutants(msa: EveAlignment, mutants: Sequence) -> Tuple[List[str], List[str]]:
    """VAE_model.py:401-450: (names, sequences); row 0 is 'wt'.  A sub-mutation to the same letter is skipped; a position outside the
    focus columns, a wrong wild-type letter, a target outside the alphabet or a string that does not parse drops the whole mutant."""
    names, seqs = ["wt"], [msa.focus_seq_trimmed]
    for mutation in mutants:
        seq = list(msa.focus_seq_trimmed)
        ok = True
        for mut in str(mutation).split(":"):
            try:
                wt_aa, pos, mut_aa = mut[0], int(mut[1:-1]), mut[-1]
            except (ValueError, IndexError):
                ok = False
                break
            if wt_aa == mut_aa:
                continue
            if pos not in msa.uniprot_focus_col_to_wt_aa_dict or msa.uniprot_focus_col_to_wt_aa_dict[pos] != wt_aa:
                ok = False
            if not msa.in_singles(mut):
                ok = False
            if not ok:
                break
            seq[msa.pos_to_letter_idx[pos][1]] = mut_aa
        if ok:
            names.append(mutation)
            seqs.append("".join(seq))
    return names, seqs


def encode_residues(seqs: Sequence[str]) -> np.ndarray:
    """uint8 [M][L]: index in the alphabet, 255 for any other letter (one_hot_3D leaves such a position all zero)."""
    table = np.full(256, NO_LETTER, dtype=np.uint8)
    table[np.frombuffer(AMINO_ACIDS.encode("ascii"), dtype=np.uint8)] = np.arange(20, dtype=np.uint8)
    L = len(seqs[0])
    if any(len(s) != L for s in seqs):
        raise ValueError("sequences differ in length")
    return table[np.frombuffer("".join(seqs).encode("ascii"), dtype=np.uint8)].reshape(len(seqs), L)


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


class EveModel(_lib.SideHandle):
    """A device-resident EVE / DeepSequence model."""

    PREFIX = "eve"

    def __init__(self, dims: dict, blob: np.ndarray, device: int = 0, precision: int = _lib.PREC_FP32):
        self.dims = dict(dims)
        d = self.dims
        c = EveConfig(abi_version=_lib.ABI_VERSION, seq_len=d["seq_len"], alphabet=20, z_dim=d["z_dim"], n_enc=len(d["enc_sizes"]),
                      n_dec=len(d["dec_sizes"]), conv_depth=d["conv_depth"], temperature=d["temperature"], sparsity_tiles=d["sparsity_tiles"],
                      enc_act=ACTS[d["enc_act"]], dec_first_act=ACTS[d["dec_first_act"]], dec_last_act=ACTS[d["dec_last_act"]],
                      precision=precision, dropout_p=d["dropout_p"])
        if len(d["enc_sizes"]) > MAX_LAYERS or len(d["dec_sizes"]) > MAX_LAYERS:
            raise _lib.PgmiError(f"at most {MAX_LAYERS} layers per stack")
        for i, v in enumerate(d["enc_sizes"]):
            c.enc_sizes[i] = v
        for i, v in enumerate(d["dec_sizes"]):
            c.dec_sizes[i] = v
        self._create(c, blob, device)
        self.L, self.z = d["seq_len"], d["z_dim"]

    def _res(self, residues):
        r = np.ascontiguousarray(residues, dtype=np.uint8)
        if r.ndim != 2 or r.shape[1] != self.L:
            raise _lib.PgmiError(f"residues must be [M, {self.L}]")
        return r

    def noise_shapes(self, M: int) -> Dict[str, Tuple[Tuple[int, ...], type]]:
        """name -> (shape, dtype) of one sample's noise tensors, in the reference's drawing order."""
        d = self.dims
        H, Cc, L = d["dec_sizes"][-1], d["conv_depth"] or 20, self.L
        drop = d["dropout_p"] > 0
        out = {"z_eps": ((M, self.z), np.float32)}
        if drop:
            out["keep0"] = ((M, self.z), np.uint8)
        fan = self.z
        for i, h in enumerate(d["dec_sizes"]):
            out[f"w_eps{i}"] = ((h, fan), np.float32)
            out[f"b_eps{i}"] = ((h,), np.float32)
            if drop:
                out[f"keep{i + 1}"] = ((M, h), np.uint8)
            fan = h
        out["wout_eps"] = ((Cc * L, H), np.float32)
        out["bout_eps"] = ((20 * L,), np.float32)
        if d["conv_depth"]:
            out["conv_eps"] = ((20, Cc, 1), np.float32)
        if d["sparsity_tiles"]:
            out["sparsity_eps"] = ((H // d["sparsity_tiles"], L), np.float32)
        if d["temperature"]:
            out["temp_eps"] = ((1,), np.float32)
        return out

    def _noise_struct(self, noise: Dict[str, np.ndarray], M: int):
        """(struct, arrays kept alive): every tensor of noise_shapes must be present with its shape."""
        s, keep_alive = EveNoise(), []
        for name, (shape, dt) in self.noise_shapes(M).items():
            if name not in noise:
                continue
            a = np.ascontiguousarray(noise[name], dtype=dt)
            if a.shape != tuple(shape):
                raise _lib.PgmiError(f"noise tensor {name}: shape {a.shape}, expected {tuple(shape)}")
            keep_alive.append(a)
            p = a.ctypes.data
            if name.startswith("keep"):
                s.keep[int(name[4:])] = p
            elif name.startswith("w_eps"):
                s.w_eps[int(name[5:])] = p
            elif name.startswith("b_eps"):
                s.b_eps[int(name[5:])] = p
            else:
                setattr(s, name, p)
        return s, keep_alive

    def encode(self, residues) -> Tuple[np.ndarray, np.ndarray]:
        r = self._res(residues)
        mu, lv = np.empty((len(r), self.z), np.float32), np.empty((len(r), self.z), np.float32)
        _lib.check(_lib.load().pgmi_eve_encode(self._h, _u8p(r), len(r), _lib.ptr(mu, _lib._f32p), _lib.ptr(lv, _lib._f32p)))
        return mu, lv

    def elbo(self, residues, seed: int = 0, sample: int = 0, row_base: int = 0, noise: Dict[str, np.ndarray] = None):
        """(elbo, bce, kld) f32 [M] of one sample; ``noise``: injected tensors (all of noise_shapes) instead of the generator."""
        r = self._res(residues)
        M = len(r)
        out = [np.empty(M, np.float32) for _ in range(3)]
        inj, alive = (None, None)
        if noise is not None:
            missing = set(self.noise_shapes(M)) - set(noise)
            if missing:
                raise _lib.PgmiError(f"injected noise lacks {sorted(missing)}")
            s, alive = self._noise_struct(noise, M)
            inj = C.byref(s)
        _lib.check(_lib.load().pgmi_eve_elbo(self._h, _u8p(r), M, row_base, seed, sample, inj, *[_lib.ptr(o, _lib._f32p) for o in out]))
        return tuple(out)

    def noise_fill(self, M: int, seed: int, sample: int, row_base: int = 0, only: Sequence[str] = None) -> Dict[str, np.ndarray]:
        """The generator's noise tensors of (seed, sample) for rows row_base .. row_base + M (``only``: a subset of the names)."""
        noise = {n: np.empty(shape, dt) for n, (shape, dt) in self.noise_shapes(M).items() if only is None or n in only}
        s, _alive = self._noise_struct(noise, M)
        _lib.check(_lib.load().pgmi_eve_noise_fill(self._h, seed, sample, row_base, M, C.byref(s)))
        return noise

    def evol_indices(self, residues, num_samples: int, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """(mean, std) f64 [M] of the ELBO over num_samples samples; row 0 is the wild type."""
        r = self._res(residues)
        mean, std = np.empty(len(r), np.float64), np.empty(len(r), np.float64)
        _lib.check(_lib.load().pgmi_eve_evol_indices(self._h, _u8p(r), len(r), num_samples, seed, _lib.ptr(mean, _lib._f64p),
                                                     _lib.ptr(std, _lib._f64p)))
        return mean, std

    def log_prior(self, residues, num_samples: int, seed: int = 0, noise: Sequence[Dict[str, np.ndarray]] = None):
        """(mean, std) f64 [L, 20] of log_softmax(decoder(z)) of one row over num_samples samples, without dropout (TranceptEVE's
        get_EVE_log_prior_single).  ``noise``: one dict per sample (noise_shapes(1) without the keep masks) instead of the generator."""
        r = self._res(np.asarray(residues).reshape(1, -1))
        mean, std = np.empty((self.L, 20), np.float64), np.empty((self.L, 20), np.float64)
        inj, alive = None, []
        if noise is not None:
            if len(noise) != num_samples:
                raise _lib.PgmiError(f"{len(noise)} noise dicts for {num_samples} samples")
            need = {n for n in self.noise_shapes(1) if not n.startswith("keep")}
            arr = (EveNoise * num_samples)()
            for j, nz in enumerate(noise):
                if need - set(nz):
                    raise _lib.PgmiError(f"injected noise of sample {j} lacks {sorted(need - set(nz))}")
                s, keep = self._noise_struct({k: v for k, v in nz.items() if k in need}, 1)
                arr[j] = s
                alive.append(keep)
            inj = C.cast(arr, C.c_void_p)
        _lib.check(_lib.load().pgmi_eve_log_prior(self._h, _u8p(r), num_samples, seed, inj, _lib.ptr(mean, _lib._f64p),
                                                  _lib.ptr(std, _lib._f64p)))
        return mean, std


def from_checkpoint(path: str, params_path: str, seq_len: int, device: int = 0) -> EveModel:
    with open(params_path) as f:
        params = json.load(f)
    d, blob = load_checkpoint(path, params, seq_len)
    return EveModel(d, blob, device=device)


def random_state_dict(d: dict, seed: int, log_var=(-6.0, -2.0), scale: float = 1.0, out_bias_std: float = 0.05) -> Dict[str, np.ndarray]:
    """Seeded weights for tests and benchmarks: Glorot-sized normals for the means (times ``scale``), the decoder's log-variances
    uniform in ``log_var`` so that the weight noise visibly matters, the output bias (the per-position letter profile) with
    ``out_bias_std``."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, shape in key_shapes(d):
        if k.startswith("decoder.") and "log_var" in k:
            a = rng.uniform(log_var[0], log_var[1], size=shape)
        elif k.endswith("temperature_scaler_mean"):
            a = np.ones(shape)
        elif k.endswith("last_hidden_layer_bias_mean"):
            a = out_bias_std * rng.standard_normal(shape)
        elif k == "encoder.fc_log_var.bias":
            a = -2.0 + 0.05 * rng.standard_normal(shape)
        elif len(shape) == 1:
            a = 0.1 + 0.05 * rng.standard_normal(shape)
        else:
            fan_out, fan_in = shape[0], int(np.prod(shape[1:]))
            a = scale * np.sqrt(2.0 / (fan_in + fan_out)) * rng.standard_normal(shape)
        out[k] = a.astype(np.float32)
    return out
