"""What the reference does with the Stage-II result: merge it with the Stage-I data, pickle it, export it in the
AMASS npz layout SOMA reads.

Mirrors, for the Stage-II side only:
  * `MoSh.mosh_stageii`            reference src/moshpp/mosh_head.py:268-301
  * `MoSh.load_as_amass_npz`       reference src/moshpp/mosh_head.py:444-541
  * `turn_fullpose_into_parts`     reference src/moshpp/tools/run_tools.py:70-85

Stage-I (marker-layout optimisation, `MoSh.mosh_stagei`, :200-266) is not part of this package: its result
(`*_stagei.pkl`, keys `markers_latent`, `latent_labels`, `betas`, `marker_meta`, `markers_latent_vids`,
`stagei_debug_details`, optional `v_template_fname`) is an input here, as a file or a dict.
"""
from __future__ import annotations

import logging
import os
import os.path as osp
import pickle
import time
from collections import namedtuple
from contextlib import contextmanager
from datetime import timedelta

import numpy as np

logger = logging.getLogger('moshpp_amd')


def _cfg_container(cfg):
    """cfg -> plain nested dict (`OmegaConf.to_container(cfg, resolve=True, enum_to_str=True)`, mosh_head.py:292-293)."""
    if hasattr(cfg, 'to_container'):
        return cfg.to_container()
    try:
        from omegaconf import OmegaConf
        return OmegaConf.to_container(cfg, resolve=True, enum_to_str=True)
    except ImportError:
        return {k: (_cfg_container(v) if hasattr(v, 'items') else v) for k, v in cfg.items()}


def _makepath(fname):
    d = osp.dirname(fname)
    if d:
        os.makedirs(d, exist_ok=True)
    return fname


def turn_fullpose_into_parts(fullpose, surface_model_type):
    """fullpose[T, 3K] -> {'root_orient', 'pose_body', 'pose_hand', 'pose_jaw', 'pose_eye'} as the AMASS npz names
    them (run_tools.py:70-85): SMPL* body = 3:66; SMPL-H hands = 66:; SMPL-X jaw 66:69, eyes 69:75, hands 75:;
    MANO hand = 3:; animal/object models keep everything after the root in 'pose_body'."""
    res = {'root_orient': fullpose[:, :3]}
    if 'smpl' in surface_model_type:
        res['pose_body'] = fullpose[:, 3:66]
    elif any(text in surface_model_type for text in ('animal', 'object')):
        res['pose_body'] = fullpose[:, 3:]
    if 'smplh' in surface_model_type:
        res['pose_hand'] = fullpose[:, 66:]
    elif 'smplx' in surface_model_type:
        res['pose_hand'] = fullpose[:, 75:]
        res['pose_jaw'] = fullpose[:, 66:69]
        res['pose_eye'] = fullpose[:, 69:75]
    elif 'mano' in surface_model_type:
        res['pose_hand'] = fullpose[:, 3:]
    return res


def run_stageii(stagei_data_or_fname, cfg, stageii_fname=None, mosh_stageii_func=None):
    """`MoSh.mosh_stageii` (mosh_head.py:268-301) without the class around it.

    Loads `stageii_fname` if it already exists (:272-274); otherwise calls `mosh_stageii_func` (default: the
    libmoshii drop-in) with exactly the keyword arguments the reference passes (:280-286), merges the Stage-I
    dict into the result (:289), records `stageii_elapsed_time` and the resolved cfg (:291-293) and pickles it.
    Returns the stageii dict."""
    if isinstance(stagei_data_or_fname, dict):
        stagei_data = stagei_data_or_fname
    else:
        if not osp.exists(stagei_data_or_fname):
            raise ValueError(f'stagei_fname results could not be found: {stagei_data_or_fname}. '
                             f'please run stagei first.')
        with open(stagei_data_or_fname, 'rb') as fh:
            stagei_data = pickle.load(fh)
    if stageii_fname and osp.exists(stageii_fname):
        logger.info(f'loading mosh stageii results from {stageii_fname}')
        with open(stageii_fname, 'rb') as fh:
            return pickle.load(fh)
    if mosh_stageii_func is None:
        from .chmosh import mosh_stageii as mosh_stageii_func
    logger.info(f'attempting mosh stageii to create {stageii_fname}')
    tm = time.time()
    stageii_data = mosh_stageii_func(mocap_fname=cfg.mocap.fname,
                                     cfg=cfg,
                                     markers_latent=stagei_data['markers_latent'],
                                     latent_labels=stagei_data['latent_labels'],
                                     betas=stagei_data['betas'],
                                     marker_meta=stagei_data['marker_meta'],
                                     v_template_fname=stagei_data.get('v_template_fname'))
    stageii_elapsed_time = time.time() - tm
    stageii_data.update(stagei_data)
    stageii_data['stageii_debug_details']['stageii_elapsed_time'] = stageii_elapsed_time
    stageii_data['stageii_debug_details']['cfg'] = _cfg_container(cfg)
    if stageii_fname:
        with open(_makepath(stageii_fname), 'wb') as fh:
            pickle.dump(stageii_data, fh)
        logger.debug(f'created stageii_fname: {stageii_fname}')
    logger.debug(f'finished mosh stageii in {timedelta(seconds=stageii_elapsed_time)}')
    return stageii_data


def prepare_stagei_frames(cfg, stagei_mocap_fnames):
    """The dispatch of `MoSh.prepare_stagei_frames` (mosh_head.py:156-197) on an explicit list of mocap files: picks the Stage-I
    frames with the configured picker (`cfg.moshpp.stagei_frame_picker.{type,num_frames,seed,least_avail_markers}`)."""
    from . import frame_picker
    from .mocap_interface import general_labels_map
    fp = cfg.moshpp.stagei_frame_picker
    common = dict(mocap_unit=cfg.mocap.unit, mocap_rotate=cfg.mocap.rotate, only_markers=cfg.mocap.only_markers,
                  only_subjects=[cfg.mocap.subject_name] if cfg.mocap.multi_subject else None,
                  exclude_markers=cfg.mocap.exclude_markers, labels_map=general_labels_map)
    if fp.type == 'random':
        return frame_picker.load_marker_sessions_random(stagei_mocap_fnames, num_frames=fp.num_frames, seed=fp.seed,
                                                        least_avail_markers=fp.least_avail_markers, **common)
    if fp.type == 'random_strict':
        return frame_picker.load_marker_sessions_random_strict(stagei_mocap_fnames, num_frames=fp.num_frames, seed=fp.seed,
                                                               least_avail_markers=fp.least_avail_markers, **common)
    if fp.type == 'manual':
        return frame_picker.load_marker_sessions_manual(stagei_mocap_fnames, **common)
    raise ValueError(f'Wrong frame_picker value: {fp.type}')


def run_stagei(cfg, stagei_mocap_fnames, stagei_fname=None, mosh_stagei_func=None):
    """`MoSh.mosh_stagei` (mosh_head.py:199-263) without the class around it: loads `stagei_fname` if it exists (checking the
    model file it was made with, :210-217), otherwise picks the frames, calls `mosh_stagei_func` (default: the libmoshii drop-in)
    with the reference's keyword arguments (:238-240), records frames / names / cfg / elapsed time (:244-249) and pickles."""
    if stagei_fname and osp.exists(stagei_fname):
        with open(stagei_fname, 'rb') as fh:
            stagei_data = pickle.load(fh)
        prev = stagei_data['stagei_debug_details']['cfg']['surface_model']['fname']
        assert prev == cfg.surface_model.fname, ValueError(
            f'The surface_model_fname used for previous stagei ({prev}) is different than the current surface model '
            f'({cfg.surface_model.type})')
        logger.info(f'loading mosh stagei results from {stagei_fname}')
        return stagei_data
    if mosh_stagei_func is None:
        from .chmosh import mosh_stagei as mosh_stagei_func
    stagei_frames, stagei_fnames = prepare_stagei_frames(cfg, stagei_mocap_fnames)
    layout_fname = cfg.dirs.marker_layout.fname
    if layout_fname and not isinstance(layout_fname, dict) and not osp.exists(layout_fname):      # mosh_head.py:227-236
        from .marker_layout import marker_labels_to_marker_layout
        from .mocap_interface import general_labels_map
        logger.debug(f'Marker layout not available. It will be produced: {layout_fname}')
        marker_labels_to_marker_layout(chosen_markers=[l for fr in stagei_frames for l in fr.keys()],
                                       marker_layout_fname=layout_fname, surface_model_type=cfg.surface_model.type,
                                       labels_map=general_labels_map,
                                       wrist_markers_on_stick=cfg.moshpp.get('wrist_markers_on_stick', False),
                                       separate_types=cfg.moshpp.get('separate_types'))
    logger.info(f'Attempting mosh stagei to create {stagei_fname}')
    tm = time.time()
    stagei_data = mosh_stagei_func(stagei_frames=stagei_frames, cfg=cfg, betas_fname=cfg.moshpp.get('betas_fname'),
                                   v_template_fname=cfg.moshpp.get('v_template_fname'))
    elapsed = time.time() - tm
    dd = stagei_data['stagei_debug_details']
    dd['stagei_fnames'] = stagei_fnames
    dd['stagei_frames'] = stagei_frames
    dd['cfg'] = _cfg_container(cfg)
    dd['stagei_elapsed_time'] = elapsed
    if stagei_fname:
        with open(_makepath(stagei_fname), 'wb') as fh:
            pickle.dump(stagei_data, fh)
        logger.debug(f'created stagei_fname: {stagei_fname}')
        if cfg.dirs.get('write_optimized_marker_layout', False):       # mosh_head.py:259-260
            dump_stagei_marker_layout(stagei_fname)
    logger.debug(f'finished mosh stagei in {timedelta(seconds=elapsed)}')
    return stagei_data


def extract_marker_layout_from_mosh(mosh_stagei, template_marker_layout_fname=None) -> dict:
    """`MoSh.extract_marker_layout_from_mosh` (mosh_head.py:562-581): the Stage-I marker layout with every label's vertex id replaced
    by the optimised one (`markers_latent_vids`); optionally on top of a template layout file."""
    import copy
    from .marker_layout import marker_layout_load
    if not isinstance(mosh_stagei, dict):
        with open(mosh_stagei, 'rb') as fh:
            mosh_stagei = pickle.load(fh)
    opt_vids = mosh_stagei['markers_latent_vids']
    meta = marker_layout_load(template_marker_layout_fname) if template_marker_layout_fname else copy.deepcopy(mosh_stagei['marker_meta'])
    for label in meta['marker_vids']:
        if label in opt_vids:
            meta['marker_vids'][label] = opt_vids[label]
    return meta


def dump_stagei_marker_layout(mosh_stagei_pkl_fname, out_marker_layout_fname=None, template_marker_layout_fname=None):
    """The json part of `MoSh.dump_stagei_marker_layout` (mosh_head.py:303-321; its mesh / c3d exports need the visualisation stack and
    are out of scope): writes the optimised layout next to the Stage-I pickle."""
    from .marker_layout import marker_layout_write
    assert str(mosh_stagei_pkl_fname).endswith('.pkl'), ValueError(f'mosh_stagei_pkl_fname should be a valid pkl file: {mosh_stagei_pkl_fname}')
    meta = extract_marker_layout_from_mosh(mosh_stagei_pkl_fname, template_marker_layout_fname)
    out = out_marker_layout_fname or str(mosh_stagei_pkl_fname).replace('.pkl', '.json')
    marker_layout_write(meta, out)
    return out


def run_moshpp_once(cfg, stagei_mocap_fnames=None):
    """The two-stage pipeline of the reference's `run_moshpp_once` (mosh_head.py:584-606) on the libmoshii drop-ins: Stage-I
    (load-or-run, pickled to cfg.dirs.stagei_fname) then, unless cfg.runtime.stagei_only, Stage-II of cfg.mocap.fname
    (cfg.dirs.stageii_fname).  `stagei_mocap_fnames`: the captures Stage-I picks its frames from (default:
    cfg.moshpp.stagei_frame_picker.stagei_mocap_fnames, else the capture itself -- the reference's per-sequence mode)."""
    fnames = stagei_mocap_fnames or cfg.moshpp.stagei_frame_picker.get('stagei_mocap_fnames') or [cfg.mocap.fname]
    stagei = run_stagei(cfg, list(fnames), stagei_fname=cfg.dirs.get('stagei_fname'))
    logger.debug('Final mosh stagei loss: {}'.format(' | '.join(
        f'{k} = {np.sum(v):2.2e}' for k, v in stagei['stagei_debug_details']['stagei_errs'].items())))
    if cfg.runtime.get('stagei_only', False):
        return stagei, None
    stageii = run_stageii(stagei, cfg, stageii_fname=cfg.dirs.get('stageii_fname'))
    logger.debug('Final mosh stageii loss: {}'.format(' | '.join(
        f'{k} = {np.sum(np.asarray(v) ** 2):2.2e}' for k, v in stageii['stageii_debug_details']['stageii_errs'].items())))
    return stagei, stageii


_STAGEI_NPZ_KEYS = ('gender', 'surface_model_type', 'markers_latent', 'latent_labels', 'markers_latent_vids', 'betas',
                    'v_template')


def load_as_amass_npz(stageii_pkl_data_or_fname, stageii_npz_fname=None, stagei_npz_fname=None,
                      include_markers=False, include_extra_details=False) -> dict:
    """`MoSh.load_as_amass_npz` (mosh_head.py:444-541): same keys, same conditions, same side files.

    Existing npz files are not overwritten (:521, 528).  The pre-2021 pickle format handled by
    `load_as_amass_npz_legacy` (:342-442) is not supported (raises)."""
    if isinstance(stageii_pkl_data_or_fname, dict):
        pkl = stageii_pkl_data_or_fname
    else:
        try:
            with open(stageii_pkl_data_or_fname, 'rb') as fh:
                pkl = pickle.load(fh)
        except UnicodeDecodeError as e:
            raise NotImplementedError('legacy (python-2 era) stageii pickles are not supported') from e
    dbg = pkl['stageii_debug_details']
    cfg = dbg['cfg']
    sm, mp = cfg['surface_model'], cfg['moshpp']
    out = {
        'gender': sm['gender'],
        'surface_model_type': sm['type'],
        'mocap_frame_rate': dbg['mocap_frame_rate'],
        'mocap_time_length': dbg['mocap_time_length'],
        'markers_latent': pkl['markers_latent'],
        'latent_labels': pkl['latent_labels'],
        'markers_latent_vids': pkl['markers_latent_vids'],
        'trans': pkl['trans'],
        'poses': pkl['fullpose'],
    }
    if include_extra_details:
        out['surface_model_fname'] = sm['fname']
    if 'v_template' in pkl['stagei_debug_details']:
        out['v_template'] = pkl['stagei_debug_details']['v_template']
    if mp['optimize_betas']:
        out['betas'] = pkl['betas'][:sm['num_betas']]
        out['num_betas'] = sm['num_betas']
    if mp['optimize_dynamics']:
        out['dmpls'] = pkl['dmpls'][:sm['num_dmpls']]        # (sic) the reference slices the frame axis here (:487)
        out['num_dmpls'] = sm['num_dmpls']
    if mp['optimize_face']:
        out['expression'] = pkl['expression'][:, :sm['num_expressions']]
        out['num_expressions'] = sm['num_expressions']
    out.update(turn_fullpose_into_parts(pkl['fullpose'], sm['type']))
    if include_markers:
        out['markers'] = dbg['markers_orig']
        out['labels'] = dbg['labels_orig']
        out['markers_obs'] = dbg['markers_obs']
        out['labels_obs'] = dbg['labels_obs']
        out['markers_sim'] = dbg['markers_sim']
        out['marker_meta'] = pkl['marker_meta']
        out['num_markers'] = out['markers'].shape[1]
    if stageii_npz_fname:
        if not osp.exists(stageii_npz_fname):
            np.savez(_makepath(str(stageii_npz_fname)), **out)
            logger.info(f'created amass_stageii_npz_fname: {stageii_npz_fname}')
        if stagei_npz_fname is None:
            stagei_npz_fname = osp.join(osp.dirname(str(stageii_npz_fname)), f"{sm['gender']}_stagei.npz")
        if not osp.exists(stagei_npz_fname):
            np.savez(_makepath(str(stagei_npz_fname)), **{k: v for k, v in out.items() if k in _STAGEI_NPZ_KEYS})
            logger.info(f'created amass_stagei_npz_fname: {stagei_npz_fname}')
    return out


# what an export decides from the Stage-II dict alone: cfg.surface_model, cfg.moshpp, kind 'expr' | 'dmpl' | None of the free block, its
# first column and size, the rows of the result to export
_StageIIPlan = namedtuple('_StageIIPlan', 'sm mp kind start count ids')


def _stageii_vertices_plan(pkl, frame_ids):
    """The _StageIIPlan of stageii_vertices (and of every other export), checked before a model is loaded or a device touched."""
    for k in ('fullpose', 'trans', 'betas', 'stageii_debug_details'):
        if k not in pkl:
            raise KeyError(f"stageii_vertices: the Stage-II data has no '{k}'")
    if 'cfg' not in pkl['stageii_debug_details']:
        raise KeyError("stageii_vertices: the Stage-II data has no stored cfg (stageii_debug_details['cfg'])")
    cfg = pkl['stageii_debug_details']['cfg']
    sm, mp = cfg['surface_model'], cfg['moshpp']
    fullpose, trans = np.asarray(pkl['fullpose']), np.asarray(pkl['trans'])
    if fullpose.ndim != 2 or trans.shape != (fullpose.shape[0], 3):
        raise ValueError(f'stageii_vertices: fullpose {fullpose.shape} / trans {trans.shape} are not [T, 3K] / [T, 3]')
    T = fullpose.shape[0]
    face, dyn = bool(mp.get('optimize_face', False)), bool(mp.get('optimize_dynamics', False))
    if face and dyn:
        raise ValueError('stageii_vertices: optimize_face and optimize_dynamics are mutually exclusive')
    if (face or 'expression' in pkl) and sm['type'] != 'smplx':
        raise ValueError(f"stageii_vertices: expression coefficients belong to smplx, the stored model type is {sm['type']}")
    if (dyn or 'dmpls' in pkl) and sm['type'] not in ('smpl', 'smplh'):
        raise ValueError(f"stageii_vertices: DMPL coefficients belong to smpl / smplh, the stored model type is {sm['type']}")
    kind, start, count = None, 0, 0
    if face:
        kind, start, count = 'expr', int(sm.get('betas_expr_start_id', 300)), int(sm.get('num_expressions', 80))
        key = 'expression'
    elif dyn:
        kind, start, count = 'dmpl', int(sm['num_betas']), int(sm.get('num_dmpls', 8))
        key = 'dmpls'
    if kind is not None:
        if key not in pkl:
            raise KeyError(f"stageii_vertices: the cfg says optimize_{'face' if face else 'dynamics'} but the data has no '{key}'")
        c = np.asarray(pkl[key])
        if c.ndim != 2 or c.shape[0] != T or c.shape[1] < count:
            raise ValueError(f"stageii_vertices: '{key}' is {c.shape}, expected [{T}, >= {count}]")
    if frame_ids is None:
        ids = np.arange(T)
    else:
        ids = np.atleast_1d(np.asarray(frame_ids))
        if ids.ndim != 1 or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError('stageii_vertices: frame_ids must be a list of integers')
        if len(ids) and (ids.min() < 0 or ids.max() >= T):
            raise IndexError(f'stageii_vertices: frame_ids outside the {T} solved frames')
    return _StageIIPlan(sm, mp, kind, start, count, ids)


def _stageii_load(stageii_data_or_fname):
    if isinstance(stageii_data_or_fname, dict):
        return stageii_data_or_fname
    with open(stageii_data_or_fname, 'rb') as fh:
        return pickle.load(fh)


def _stageii_export_inputs(pkl, plan, surface_model):
    """(surface_model, shapedirs, betas, fullpose[ids], trans[ids], coefficients | None) of a planned export: what the model handle
    of stageii_vertices / stageii_virtual_markers is created from -- no device touched yet."""
    sm, mp, kind, start, count, ids = plan
    from .models import load_surface_model
    if surface_model is None:
        surface_model = load_surface_model(surface_model_fname=sm['fname'], surface_model_type=sm['type'],
                                           pose_hand_prior_fname=mp.get('pose_hand_prior_fname'),
                                           use_hands_mean=sm.get('use_hands_mean', False), dof_per_hand=sm.get('dof_per_hand', 12),
                                           v_template_fname=pkl.get('v_template_fname'))
    K = surface_model.K
    fullpose = np.asarray(pkl['fullpose'], dtype=np.float64)
    if fullpose.shape[1] != 3 * K:
        raise ValueError(f'stageii_vertices: fullpose has {fullpose.shape[1]} columns, the model {3 * K}')
    shapedirs = np.asarray(surface_model.shapedirs, dtype=np.float64)
    if kind == 'dmpl':
        if shapedirs.shape[2] < start + count:
            shapedirs = np.concatenate([shapedirs, np.zeros(shapedirs.shape[:2] + (start + count - shapedirs.shape[2],))], axis=2)
        if sm.get('dmpl_fname'):
            from .chmosh import read_dmpl_pcs
            shapedirs = shapedirs.copy()
            shapedirs[:, :, start:start + count] = np.asarray(read_dmpl_pcs(sm['dmpl_fname']), dtype=np.float64)[:, :, :count]
    if kind is not None and start + count > shapedirs.shape[2]:
        raise ValueError(f'stageii_vertices: the free block [{start}, {start + count}) exceeds the {shapedirs.shape[2]} shape '
                         f'coefficients of the model')
    nb = int(sm['num_betas'])
    betas = np.asarray(pkl['betas'], dtype=np.float64).ravel()
    b = np.zeros(shapedirs.shape[2])
    b[:nb] = betas[:nb]                                   # as mosh_stageii applies them
    coef = None
    if kind is not None:   # stored: the frozen betas of those columns + the solved offsets
        coef = np.asarray(pkl['expression' if kind == 'expr' else 'dmpls'], dtype=np.float64)[ids, :count] - b[start:start + count]
    return surface_model, shapedirs, b, fullpose[ids], np.asarray(pkl['trans'], dtype=np.float64)[ids], coef


def _stageii_device(surface_model, shapedirs, b, kind, start, count):
    from . import capi
    K = surface_model.K
    # the pickle holds the FULL pose: every joint's rotation vector is a pose variable of this handle (no hand-PCA map)
    dev = capi.Model(surface_model.v_template, shapedirs, surface_model.posedirs, surface_model.weights, surface_model.J_regressor,
                     surface_model.parents, 3 * K, 0)
    try:
        dev.set_betas(b)
        if kind is not None:
            dev.set_free_shape(start, count)
    except Exception:
        dev.close()
        raise
    return dev


def _need_model_faces(who, surface_model):
    if getattr(surface_model, 'f', None) is None:
        what = 'return_normals needs a surface model with faces (f)' if who == 'stageii_vertices' else 'the surface model has no faces (f)'
        raise ValueError(f'{who}: {what}')


def _need_model_vertices(vids, surface_model):
    if len(vids) and vids.max() >= surface_model.V:
        raise ValueError(f'stageii_virtual_markers: vertex ids beyond the {surface_model.V} vertices of the model')


@contextmanager
def _stageii_session(pkl, plan, surface_model, who, faces=False, vids=None):
    """The model handle of a planned export, open for the `with` block: (handle, surface model (loaded from the stored cfg where none is
    given), fullpose[ids], trans[ids], coefficients[ids] | None).  faces: the model must bring its triangles, which the handle then
    holds; vids: vertex ids that must lie on the model.  Both are refused before a device is touched."""
    surface_model, shapedirs, b, fullpose, trans, coef = _stageii_export_inputs(pkl, plan, surface_model)
    if faces:
        _need_model_faces(who, surface_model)
    if vids is not None:
        _need_model_vertices(vids, surface_model)
    dev = _stageii_device(surface_model, shapedirs, b, plan.kind, plan.start, plan.count)
    try:
        if faces:
            dev.set_faces(surface_model.f)
        yield dev, surface_model, fullpose, trans, coef
    finally:
        dev.close()


def _observed_points(pkl, ids, who, required, with_simulated=False):
    """(labels, observed[len(ids), M, 3], simulated[len(ids), M, 3] | None): the ragged markers_obs (and, with_simulated, markers_sim) of
    a Stage-II result on the rows `ids`, laid out over latent_labels -- or, without them, the labels in the order the frames first name
    them -- NaN where a label is not observed.  A result without markers_obs / labels_obs: a KeyError if they are `required`, no points
    otherwise."""
    dbg = pkl['stageii_debug_details']
    src = dbg if 'markers_obs' in dbg else pkl          # (load_as_amass_npz(include_markers=True) lifts them to the top level)
    for k in ('markers_obs', 'labels_obs'):
        if k not in src:
            if required:
                raise KeyError(f"{who}: the Stage-II data has no '{k}'")
            return [], np.zeros((len(ids), 0, 3)), None
    T = np.asarray(pkl['fullpose']).shape[0]
    if len(src['markers_obs']) != T or len(src['labels_obs']) != T:
        raise ValueError(f"{who}: markers_obs / labels_obs hold {len(src['markers_obs'])} / {len(src['labels_obs'])} frames, the result {T}")
    labels = list(pkl['latent_labels']) if 'latent_labels' in pkl else list(dict.fromkeys(l for row in src['labels_obs'] for l in row))
    from .chmosh import pack_observed_markers
    try:
        obs = pack_observed_markers(src['markers_obs'], src['labels_obs'], labels, ids)
        sim = pack_observed_markers(src['markers_sim'], src['labels_obs'], labels, ids) if with_simulated and 'markers_sim' in src else None
    except ValueError as e:
        raise ValueError(f'{who}: {e}') from None
    return labels, obs, sim


def stageii_vertices(stageii_data_or_fname, surface_model=None, frame_ids=None, dtype=np.float32, return_normals=False):
    """verts[T, V, 3]: the meshes a Stage-II result (pickle file name or dict) describes, frame by frame -- pose, translation,
    Stage-I betas AND, where the solve freed them, the per-frame expression (optimize_face, SMPL-X) or DMPL coefficients
    (optimize_dynamics, SMPL / SMPL-H): rest positions and joints move with them exactly as they did in the solve, so the mesh
    carries the solve's simulated markers.  Every other result (body / finger solves, MANO, the animal models) is a plain export.

    surface_model: a models.SurfaceModel; default: the model file named by the stored cfg.  With optimize_dynamics the DMPL
    directions of cfg.surface_model.dmpl_fname replace shapedirs[:, :, num_betas : num_betas + num_dmpls] as in the solve; a cfg
    without dmpl_fname means the given surface_model already holds them there.  frame_ids: rows of the result (default: all).
    dtype float32: the batched export kernels (|error| <= 2e-5 m); float64: the reference-precision kernel.
    return_normals: (verts, normals) -- the area-weighted unit vertex normals [T, V, 3] of the same frames and dtype, computed on
    the device from the exported buffer (the model needs its triangles `f`)."""
    pkl = _stageii_load(stageii_data_or_fname)
    plan = _stageii_vertices_plan(pkl, frame_ids)
    if return_normals and surface_model is not None:
        _need_model_faces('stageii_vertices', surface_model)
    with _stageii_session(pkl, plan, surface_model, 'stageii_vertices', faces=return_normals) as (dev, _, fullpose, trans, coef):
        export = dev.lbs_forward_with_normals if return_normals else dev.lbs_forward
        return export(fullpose, trans, dtype=dtype, shape=coef)


DEFAULT_M2B_DISTANCE = 0.0095     # prepare_mosh_markers_latent's default distance from skin (chmosh.py:59)


def _virtual_marker_layout(marker_layout):
    """(labels, vids[M], m2b[M], surface_model_type | None) of a layout: a json file name, the dict marker_layout_load returns, or a
    plain label -> vertex id dict (0.0095 m for every marker).  Distances as prepare_mosh_markers_latent takes them
    (chmosh.py:57-64): 0.0095 by default, m2b_distance[type] under each marker_type_mask."""
    if isinstance(marker_layout, (str, os.PathLike)):
        from .marker_layout import marker_layout_load
        marker_layout = marker_layout_load(str(marker_layout))
    if not isinstance(marker_layout, dict) or not len(marker_layout):
        raise ValueError('stageii_virtual_markers: marker_layout must be a layout file name, a loaded layout or a label -> vertex id dict')
    if 'marker_vids' in marker_layout:
        meta = marker_layout
        labels = list(meta['marker_vids'].keys())
        raw = list(meta['marker_vids'].values())
        model_type = meta.get('surface_model_type')
    else:
        meta = None
        labels = list(marker_layout.keys())
        raw = list(marker_layout.values())
        model_type = None
    if any(isinstance(v, (list, tuple, np.ndarray)) for v in raw):
        raise ValueError('stageii_virtual_markers: a superset layout (several vertex ids per label) places no single marker; '
                         'pick one vertex per label first')
    vids = np.asarray(raw)
    if not np.issubdtype(vids.dtype, np.integer) or (len(vids) and vids.min() < 0):
        raise ValueError('stageii_virtual_markers: vertex ids must be non-negative integers')
    m2b = np.full(len(labels), DEFAULT_M2B_DISTANCE)
    if meta is not None:
        for mask_type, mask in meta.get('marker_type_mask', {}).items():
            m2b[np.asarray(mask, dtype=bool)] = float(meta['m2b_distance'][mask_type])
    return labels, vids.astype(np.int32), m2b, model_type


def _stageii_virtual_markers_plan(pkl, marker_layout, surface_model, frame_ids, out_fname):
    """Every refusal of stageii_virtual_markers that needs no model file and no device."""
    plan = _stageii_vertices_plan(pkl, frame_ids)
    labels, vids, m2b, layout_type = _virtual_marker_layout(marker_layout)
    if layout_type is not None and layout_type != plan.sm['type']:
        raise ValueError(f"stageii_virtual_markers: the layout is for {layout_type}, the Stage-II result for {plan.sm['type']}")
    if out_fname is not None and not str(out_fname).endswith(('.c3d', '.npz')):
        raise ValueError(f'stageii_virtual_markers: out_fname must end in .c3d or .npz: {out_fname}')
    if out_fname is not None and 'mocap_frame_rate' not in pkl['stageii_debug_details']:
        raise KeyError("stageii_virtual_markers: the Stage-II data stores no frame rate (stageii_debug_details['mocap_frame_rate']) "
                       "to write the file with")
    if surface_model is not None:
        _need_model_faces('stageii_virtual_markers', surface_model)
        _need_model_vertices(vids, surface_model)
    return plan, labels, vids, m2b


def stageii_virtual_markers(stageii_data_or_fname, marker_layout, surface_model=None, frame_ids=None, dtype=np.float32, out_fname=None):
    """dict(markers[T, M, 3], labels, vids, m2b): the markers a layout would carry on every frame of a Stage-II result --
    vertex + vertex normal x distance-from-skin, the reference's rule for ONE canonical body (prepare_mosh_markers_latent,
    chmosh.py:57-67; marker_layout_to_c3d, marker_layout/edit_tools.py) on each solved frame's mesh: synthetic mocap, re-targeting a
    capture to another layout, filling markers the capture never had.  The meshes stay on the device.

    marker_layout: a layout json file name, the dict marker_layout_load returns, or a plain label -> vertex id dict (0.0095 m for
    every marker).  surface_model / frame_ids / dtype / per-frame expression and DMPL coefficients: as in stageii_vertices.
    out_fname: '.c3d' (write_mocap_c3d) or '.npz' (markers, labels, frame_rate as MocapSession reads them), at the frame rate the
    Stage-II result stores (a result without one is a KeyError, raised before any work)."""
    pkl = _stageii_load(stageii_data_or_fname)
    plan, labels, vids, m2b = _stageii_virtual_markers_plan(pkl, marker_layout, surface_model, frame_ids, out_fname)
    with _stageii_session(pkl, plan, surface_model, 'stageii_virtual_markers', faces=True, vids=vids) as (dev, _, fullpose, trans, coef):
        markers = dev.virtual_markers(fullpose, trans, vids, m2b, dtype=dtype, shape=coef)
    if out_fname is not None:
        rate = float(pkl['stageii_debug_details']['mocap_frame_rate'])
        if str(out_fname).endswith('.c3d'):
            from .mocap_interface import write_mocap_c3d
            write_mocap_c3d(markers, labels, _makepath(str(out_fname)), frame_rate=rate)
        else:
            np.savez(_makepath(str(out_fname)), markers=markers, labels=labels, frame_rate=rate)
    return dict(markers=markers, labels=labels, vids=vids, m2b=m2b)


def _stageii_marker_skin_distance_plan(pkl, surface_model, frame_ids):
    """Every refusal of stageii_marker_skin_distance that needs no model file and no device; (plan, labels, points[T, M, 3])."""
    plan = _stageii_vertices_plan(pkl, frame_ids)
    labels, points, _ = _observed_points(pkl, plan.ids, 'stageii_marker_skin_distance', required=True)
    if surface_model is not None:
        _need_model_faces('stageii_marker_skin_distance', surface_model)
    return plan, labels, points


def stageii_marker_skin_distance(stageii_data_or_fname, surface_model=None, frame_ids=None, dtype=np.float32):
    """How far from the solved skin every observed marker sits, on every frame, and on which side -- the reference's
    PtsToMesh(signed=True) (scan2mesh/mesh_distance_main.py:158-297) between the markers_obs a Stage-II result stores and the meshes
    it describes (pose, translation, betas and per-frame expression / DMPL coefficients as in stageii_vertices); the meshes stay on the
    device.  Markers that sank into the body, swapped labels, a layout whose distance from the skin does not fit the subject and
    frames where the fit drifts all show here.

    Returns dict(labels, distance[T, M] signed metres (NaN where a label is not observed on a frame), face[T, M], part[T, M]
    (0 interior, 1-3 edges, 4-6 vertices; -1 unobserved), frame_ids, summary): summary[label] = dict(count, median, p5, p95,
    negative_share) over the label's observed frames.  surface_model / frame_ids / dtype: as in stageii_vertices."""
    pkl = _stageii_load(stageii_data_or_fname)
    plan, labels, points = _stageii_marker_skin_distance_plan(pkl, surface_model, frame_ids)
    with _stageii_session(pkl, plan, surface_model, 'stageii_marker_skin_distance', faces=True) as (dev, _, fullpose, trans, coef):
        res = dev.marker_surface_distance(fullpose, trans, points, shape=coef, dtype=dtype)
    from .chmosh import skin_distance_summary
    return dict(labels=labels, distance=res.distance, face=res.face, part=res.part, frame_ids=np.asarray(plan.ids),
                summary=skin_distance_summary(res.distance, labels))


def _stageii_joints_plan(pkl, frame_ids, out_fname):
    """Every refusal of stageii_joints that needs no model file and no device; (plan, frame rate | None)."""
    plan = _stageii_vertices_plan(pkl, frame_ids)
    rate = pkl['stageii_debug_details'].get('mocap_frame_rate')
    if out_fname is not None:
        if not str(out_fname).endswith('.npz'):
            raise ValueError(f'stageii_joints: out_fname must end in .npz: {out_fname}')
        if rate is None:
            raise KeyError("stageii_joints: the Stage-II data stores no frame rate (stageii_debug_details['mocap_frame_rate']) "
                           "to write the file with")
        if osp.exists(str(out_fname)):
            raise FileExistsError(f'stageii_joints: {out_fname} exists; remove it or choose another name')
    return plan, None if rate is None else float(rate)


def stageii_joints(stageii_data_or_fname, surface_model=None, frame_ids=None, dtype=np.float64, return_rotations=False, out_fname=None):
    """The skeleton animation a Stage-II result (pickle file name or dict) is: dict(joints[T, K, 3] world joint positions with the
    translation, rotations[T, K, 3, 3] world joint rotations (with return_rotations), parents[K], frame_ids, mocap_frame_rate (None
    where the result stores none), surface_model_type) -- the reference's J_transformed / A_global (smpl_fast_derivatives.py:218-229)
    from the kinematic chain itself, not regressed from posed vertices: right with pose correctives active, and following the per-frame
    expression / DMPL coefficients where the solve freed them.  For retargeting, MPJPE-style evaluation, contact and velocity analysis,
    skeleton viewers.

    surface_model / frame_ids: as in stageii_vertices.  dtype float64 or float32 (computed in float64, rounded once).
    out_fname: a '.npz' that receives the same entries; its directory is created, an existing file is refused (before any work)."""
    pkl = _stageii_load(stageii_data_or_fname)
    plan, rate = _stageii_joints_plan(pkl, frame_ids, out_fname)
    with _stageii_session(pkl, plan, surface_model, 'stageii_joints') as (dev, surface_model, fullpose, trans, coef):
        res = dev.posed_joints(fullpose, trans, shape=coef, dtype=dtype, return_rotations=return_rotations)
    out = dict(joints=res[0] if return_rotations else res)
    if return_rotations:
        out['rotations'] = res[1]
    out.update(parents=np.asarray(surface_model.parents, dtype=np.int32), frame_ids=np.asarray(plan.ids), mocap_frame_rate=rate,
               surface_model_type=plan.sm['type'])
    if out_fname is not None:
        np.savez(_makepath(str(out_fname)), **out)
    return out


PREVIEW_BATCH = 32                # frames rendered per call: bounds the host memory a long sequence needs beside the images themselves


def _stageii_preview_plan(pkl, surface_model, frame_ids, out_dir, size, contact_sheet_columns):
    """Every refusal of stageii_preview that needs no model file and no device; (plan, observed[T, M, 3], simulated[T, M, 3] or None,
    file names, contact-sheet file name or None)."""
    plan = _stageii_vertices_plan(pkl, frame_ids)
    ids = plan.ids
    try:
        W, H = (int(x) for x in size)
    except (TypeError, ValueError):
        raise ValueError(f'stageii_preview: size must be (width, height), got {size!r}') from None
    if not (1 <= W <= 4096 and 1 <= H <= 4096):
        raise ValueError(f'stageii_preview: width and height must be within 1 .. 4096, got {W} x {H}')
    if contact_sheet_columns is not None and int(contact_sheet_columns) < 1:
        raise ValueError(f'stageii_preview: contact_sheet_columns must be >= 1, got {contact_sheet_columns!r}')
    if len(ids) == 0:
        raise ValueError('stageii_preview: no frame to render')
    if surface_model is not None:
        _need_model_faces('stageii_preview', surface_model)
    _, obs, sim = _observed_points(pkl, ids, 'stageii_preview', required=False, with_simulated=True)
    fnames, sheet = [], None
    if out_dir is not None:
        fnames = [osp.join(str(out_dir), 'frame_%06d.png' % int(f)) for f in ids]
        if len(set(fnames)) != len(fnames):
            raise ValueError('stageii_preview: frame_ids names a frame twice, its file would be written twice')
        if contact_sheet_columns is not None:
            sheet = osp.join(str(out_dir), 'contact_sheet.png')
        for fn in fnames + ([sheet] if sheet else []):
            if osp.exists(fn):
                raise FileExistsError(f'stageii_preview: {fn} exists; remove it or choose another directory')
    return plan, obs, sim, fnames, sheet


def stageii_preview(stageii_data_or_fname, out_dir=None, surface_model=None, frame_ids=None, size=(512, 512), view='front',
                    contact_sheet_columns=None, up='z', marker_radius=0.0095):
    """Pictures of a Stage-II result (pickle file name or dict), what the reference shows while it solves (tools/visualization.py:96-130):
    the solved body of every frame with the observed markers (red) and, where the result stores them, the solve's simulated markers
    (blue), rasterised on the device by the rendering rules of include/moshii.h; the meshes never reach the host.

    One camera for the whole sequence (preview.preview_camera of the frames' posed joints, from `view` with the world axis `up` upwards).
    out_dir: receives frame_%06d.png (the number is the row of the result) and, with contact_sheet_columns, contact_sheet.png; it is
    created; an existing file is refused before any work.  Frames are rendered PREVIEW_BATCH at a time.
    Returns dict(images[T, H, W, 3] uint8, camera, frame_ids, fnames, contact_sheet (the image, or None), contact_sheet_fname).
    surface_model / frame_ids: as in stageii_vertices."""
    from . import preview, png_io
    pkl = _stageii_load(stageii_data_or_fname)
    plan, obs, sim, fnames, sheet_fname = _stageii_preview_plan(pkl, surface_model, frame_ids, out_dir, size, contact_sheet_columns)
    ids = plan.ids
    points = obs if sim is None else np.concatenate([obs, sim], axis=1)
    N = points.shape[1]
    prgb = np.array([preview.OBSERVED_RGB] * obs.shape[1] + [preview.SIMULATED_RGB] * (N - obs.shape[1]), dtype=np.uint8).reshape(N, 3)
    W, H = int(size[0]), int(size[1])
    images = np.zeros((len(ids), H, W, 3), dtype=np.uint8)
    with _stageii_session(pkl, plan, surface_model, 'stageii_preview', faces=True) as (dev, _, fullpose, trans, coef):
        camera = preview.preview_camera(dev.posed_joints(fullpose, trans, shape=coef), (W, H), view=view, up=up)
        for a in range(0, len(ids), PREVIEW_BATCH):
            z = slice(a, a + PREVIEW_BATCH)
            images[z] = dev.render_posed(fullpose[z], trans[z], camera, (W, H), points=points[z] if N else None, point_rgb=prgb if N else None,
                                         point_radius=float(marker_radius) if N else None, shape=None if coef is None else coef[z],
                                         outputs=('rgb',))['rgb']
    sheet = preview.contact_sheet(images, contact_sheet_columns) if contact_sheet_columns is not None else None
    for fn, img in zip(fnames, images):
        png_io.write_png(_makepath(fn), img)
    if sheet_fname is not None:
        png_io.write_png(_makepath(sheet_fname), sheet)
    return dict(images=images, camera=camera, frame_ids=np.asarray(ids), fnames=fnames, contact_sheet=sheet, contact_sheet_fname=sheet_fname)
