"""What the create entries of the seven handles outside pgmi_model accept and refuse, and the life of their Python objects: EVE,
ProteinMPNN, UniRep, S2F, S3F, CARP and ProtSSN.  Every case is a refusal or a create + destroy on the smallest seeded weights of the
model's own GPU test file; nothing is run on a handle.  The refusals go through ctypes, because the Python classes catch a wrong
blob size themselves and never show the handle the entry leaves behind.

Pinned per handle: a blob one element short and a device index one past the last are PGMI_EINVAL with the out handle NULL; CARP,
UniRep and ProtSSN refuse a blob with a NaN, EVE, ProteinMPNN and S2F take it (the weights are uploaded as they are); an object
closes twice and dies without an error and has a non-null profiling handle while it lives."""
import ctypes as C
import functools

import numpy as np
import pytest

import mpnn_cases as mc
from proteingym_amd import _lib, carp, eve, mpnn, protssn, s2f, s3f, synthetic as S, unirep

pytestmark = pytest.mark.gpu

ESM_CFG = dict(S.ESM2_650M, layers=2, embed_dim=128, heads=2, ffn_dim=256)
EVE_DIMS = dict(seq_len=21, z_dim=50, enc_sizes=[2000, 1000, 300], dec_sizes=[300, 1000, 2000], conv_depth=40, temperature=1,
                sparsity_tiles=0, enc_act="relu", dec_first_act="relu", dec_last_act="relu", dropout_p=0.1)
CARP_D, CARP_LAYERS = 64, 3
UR_H = 64
SSN_D, SSN_H, SSN_LAYERS = 64, 48, 2
SCANS = {"carp": True, "unirep": True, "protssn": True, "eve": False, "mpnn": False, "s2f": False}     # is a NaN in the blob refused
HANDLES = ("carp", "eve", "mpnn", "protssn", "s2f", "s3f", "unirep")


@functools.lru_cache(maxsize=None)
def carp_checkpoint():
    return carp.random_checkpoint(11 + CARP_D, CARP_D, CARP_LAYERS, False)


@functools.lru_cache(maxsize=None)
def gvp_state(module):
    return module.random_state_dict(5, ESM_CFG, esm_blob=S.random_weights(ESM_CFG, seed=3))


@functools.lru_cache(maxsize=None)
def spec(name):
    """(create entry, destroy entry, config struct, blob, the arguments between the blob and the device)"""
    if name == "carp":
        ck = carp_checkpoint()
        s = carp.check_checkpoint(ck)
        cfg = carp.CarpConfig(abi_version=_lib.ABI_VERSION, d_model=s.d_model, d_hidden=s.d_hidden, n_layers=s.n_layers,
                              kernel_size=s.kernel_size, r=s.r, vocab=s.vocab, mask_id=carp.MASK_ID, precision=_lib.PREC_F16X3, max_rows=0,
                              ln_eps=carp.LN_EPS)
        return "pgmi_carp_create", "pgmi_carp_destroy", cfg, carp.blob_from_state(ck["model_state_dict"], s), ()
    if name == "eve":
        d = EVE_DIMS
        cfg = eve.EveConfig(abi_version=_lib.ABI_VERSION, seq_len=d["seq_len"], alphabet=20, z_dim=d["z_dim"], n_enc=len(d["enc_sizes"]),
                            n_dec=len(d["dec_sizes"]), conv_depth=d["conv_depth"], temperature=d["temperature"],
                            sparsity_tiles=d["sparsity_tiles"], enc_act=eve.ACTS[d["enc_act"]], dec_first_act=eve.ACTS[d["dec_first_act"]],
                            dec_last_act=eve.ACTS[d["dec_last_act"]], precision=_lib.PREC_FP32, dropout_p=d["dropout_p"])
        for i, v in enumerate(d["enc_sizes"]):
            cfg.enc_sizes[i] = v
        for i, v in enumerate(d["dec_sizes"]):
            cfg.dec_sizes[i] = v
        return "pgmi_eve_create", "pgmi_eve_destroy", cfg, eve.blob_from_state_dict(eve.random_state_dict(d, seed=17), d), ()
    if name == "mpnn":
        cfg = mpnn.MpnnConfig(abi_version=_lib.ABI_VERSION, hidden=mpnn.HIDDEN, num_edges=mc.NUM_EDGES, enc_layers=3, dec_layers=3,
                              precision=_lib.PREC_FP32)
        return "pgmi_mpnn_create", "pgmi_mpnn_destroy", cfg, mpnn.blob_from_state_dict(mpnn.random_state_dict(7)), ()
    if name == "unirep":
        cfg = unirep.UniRepConfig(abi_version=_lib.ABI_VERSION, hidden=UR_H, vocab=unirep.VOCAB, precision=_lib.PREC_F16X3, max_rows=0)
        return "pgmi_unirep_model_create", "pgmi_unirep_destroy", cfg, unirep.blob_from_arrays(unirep.random_arrays(3, UR_H)), ()
    if name == "protssn":
        cfg = protssn.ProtssnConfig(abi_version=_lib.ABI_VERSION, node_in=SSN_D, hidden=SSN_H, layers=SSN_LAYERS,
                                    edge_attr_dim=protssn.EDGE_ATTR_DIM, precision=_lib.PREC_F16X3, edge_chunk=0)
        sd = protssn.random_state_dict(5, SSN_D, SSN_H, gain=0.5, layers=SSN_LAYERS, bias_std=0.02)
        return "pgmi_protssn_create", "pgmi_protssn_destroy", cfg, protssn.pack(sd, SSN_D, SSN_H, SSN_LAYERS), ()
    # S2F / S3F: no ESM2 model (a handle with one takes the model's device, whatever the argument says)
    if name == "s2f":
        cfg = s2f.make_config(ESM_CFG["embed_dim"])
        return "pgmi_s2f_create", "pgmi_s2f_destroy", cfg, s2f.pack(gvp_state(s2f), ESM_CFG)[1], (None,)
    assert name == "s3f"
    cfg = s3f.S3fConfig(s2f=s2f.make_config(ESM_CFG["embed_dim"]), surf_feat=s3f.SURF_IN[0], surf_res_neighbors=s3f.SURF_RES_NEIGHBORS,
                        surf_neighbors=s3f.SURF_NEIGHBORS)
    return "pgmi_s3f_create", "pgmi_s3f_destroy", cfg, s3f.pack(gvp_state(s3f), ESM_CFG)[1], (None,)


def create(lib, name, blob, device=0):
    """(return code, out handle, message) of the create entry on `blob`"""
    entry, _, cfg, _, mid = spec(name)
    w = _lib.as_f32(blob)
    h = C.c_void_p()
    rc = getattr(lib, entry)(C.byref(cfg), _lib.ptr(w, _lib._f32p), w.size, *mid, device, C.byref(h))
    return rc, h, lib.pgmi_last_error().decode(errors="replace")


@pytest.mark.parametrize("name", HANDLES)
def test_short_blob_is_refused(lib, name):
    rc, h, msg = create(lib, name, _lib.as_f32(spec(name)[3])[:-1])
    assert rc == _lib.EINVAL and "weight blob has" in msg and not h.value, (rc, msg)


@pytest.mark.parametrize("name", HANDLES)
def test_device_past_the_last_is_refused(lib, name):
    rc, h, msg = create(lib, name, spec(name)[3], device=lib.pgmi_device_count())
    assert rc == _lib.EINVAL and "out of range" in msg and not h.value, (rc, msg)


@pytest.mark.parametrize("name", sorted(SCANS))
def test_nan_in_the_blob(lib, name):
    blob = _lib.as_f32(spec(name)[3]).copy()
    blob[-1] = np.nan
    rc, h, msg = create(lib, name, blob)
    if SCANS[name]:
        assert rc == _lib.EINVAL and "not finite" in msg and not h.value, (rc, msg)
    else:
        assert rc == 0 and h.value, (rc, msg)
        getattr(lib, spec(name)[1])(h)


def build(name):
    if name == "carp":
        return carp.CarpModel(carp_checkpoint()), [()]
    if name == "eve":
        return eve.EveModel(EVE_DIMS, spec("eve")[3]), [()]
    if name == "mpnn":
        return mpnn.MpnnModel(spec("mpnn")[3], num_edges=mc.NUM_EDGES), [()]
    if name == "unirep":
        return unirep.UniRepModel(unirep.random_arrays(3, UR_H)), [()]
    if name == "protssn":
        return protssn.ProtSSN(spec("protssn")[3], SSN_D, SSN_H, SSN_LAYERS), [()]
    if name == "s2f":
        return s2f.from_state_dict(gvp_state(s2f), ESM_CFG), [()]
    return s3f.from_state_dict(gvp_state(s3f), ESM_CFG), [(0,), (1,)]


@pytest.mark.parametrize("name", HANDLES)
def test_object_life(lib, name):
    m, parts = build(name)
    accessors = [getattr(m, a) for a in ("profile_handle", "profile_view") if hasattr(m, a)]
    assert accessors
    for get in accessors:
        for part in parts:
            p = get(*part)
            assert (p if isinstance(p, C.c_void_p) else p._h).value
    esm = getattr(m, "esm", None)
    m.close()
    m.close()
    del m
    if esm is not None:
        esm.close()
