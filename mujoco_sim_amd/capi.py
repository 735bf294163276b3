"""ctypes view of the C ABI declared in include/mjhip.h.

The Python layer is plumbing for tests and bench.py; the product is the C-ABI
shared library `libmjhip.so` (HIP kernels + host C++).  Nothing here computes
physics, and there is no CPU fallback: if the library is missing the import
fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MJHIP_LIB") or os.path.join(_HERE, "libmjhip.so")   # (MJHIP_LIB: A/B builds of the library)

c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)


class Option(C.Structure):
    _fields_ = [
        ("timestep", C.c_double),
        ("gravity", C.c_double * 3),
        ("iterations", C.c_int),
        ("tolerance", C.c_double),
        ("impratio", C.c_double),
        ("noslip_iterations", C.c_int),
        ("disableflags", C.c_int),
        ("noslip_tolerance", C.c_double),
    ]


_INT_SIZES = ["nq", "nv", "nbody", "njnt", "ngeom", "neq", "npair", "nM", "ntree", "nexclude", "maxcon", "maxefc", "nmesh", "nmeshvert"]

# (name, ctype, length expression) in the exact order of struct mjh_model
_ARRAYS = [
    ("body_parentid", "i", "nbody"), ("body_rootid", "i", "nbody"), ("body_weldid", "i", "nbody"),
    ("body_jntadr", "i", "nbody"), ("body_jntnum", "i", "nbody"), ("body_dofadr", "i", "nbody"),
    ("body_dofnum", "i", "nbody"), ("body_treeid", "i", "nbody"), ("body_level", "i", "nbody"),
    ("body_geomadr", "i", "nbody"), ("body_geomnum", "i", "nbody"),
    ("body_pos", "d", "3*nbody"), ("body_quat", "d", "4*nbody"), ("body_ipos", "d", "3*nbody"),
    ("body_iquat", "d", "4*nbody"), ("body_mass", "d", "nbody"), ("body_inertia", "d", "3*nbody"),
    ("body_gravcomp", "d", "nbody"), ("body_invweight0", "d", "2*nbody"),
    ("jnt_type", "i", "njnt"), ("jnt_qposadr", "i", "njnt"), ("jnt_dofadr", "i", "njnt"),
    ("jnt_bodyid", "i", "njnt"), ("jnt_limited", "i", "njnt"),
    ("jnt_pos", "d", "3*njnt"), ("jnt_axis", "d", "3*njnt"), ("jnt_stiffness", "d", "njnt"),
    ("jnt_range", "d", "2*njnt"), ("jnt_margin", "d", "njnt"), ("jnt_solref", "d", "2*njnt"),
    ("jnt_solimp", "d", "5*njnt"), ("qpos0", "d", "nq"), ("qpos_spring", "d", "nq"),
    ("dof_bodyid", "i", "nv"), ("dof_jntid", "i", "nv"), ("dof_parentid", "i", "nv"),
    ("dof_Madr", "i", "nv"), ("dof_treeid", "i", "nv"),
    ("dof_armature", "d", "nv"), ("dof_damping", "d", "nv"), ("dof_frictionloss", "d", "nv"),
    ("dof_invweight0", "d", "nv"), ("dof_solref", "d", "2*nv"), ("dof_solimp", "d", "5*nv"),
    ("tree_dofadr", "i", "ntree"), ("tree_dofnum", "i", "ntree"), ("tree_bodyid", "i", "ntree"),
    ("geom_type", "i", "ngeom"), ("geom_bodyid", "i", "ngeom"), ("geom_condim", "i", "ngeom"),
    ("geom_contype", "i", "ngeom"), ("geom_conaffinity", "i", "ngeom"), ("geom_priority", "i", "ngeom"),
    ("geom_pos", "d", "3*ngeom"), ("geom_quat", "d", "4*ngeom"), ("geom_size", "d", "3*ngeom"),
    ("geom_rbound", "d", "ngeom"), ("geom_friction", "d", "3*ngeom"), ("geom_solmix", "d", "ngeom"),
    ("geom_solref", "d", "2*ngeom"), ("geom_solimp", "d", "5*ngeom"), ("geom_margin", "d", "ngeom"),
    ("geom_gap", "d", "ngeom"),
    ("pair_geom1", "i", "npair"), ("pair_geom2", "i", "npair"),
    ("eq_type", "i", "neq"), ("eq_obj1id", "i", "neq"), ("eq_obj2id", "i", "neq"), ("eq_active", "i", "neq"),
    ("eq_data", "d", "11*neq"), ("eq_solref", "d", "2*neq"), ("eq_solimp", "d", "5*neq"),
    ("geom_dataid", "i", "ngeom"), ("mesh_vertadr", "i", "nmesh"), ("mesh_vertnum", "i", "nmesh"),
    ("mesh_vert", "d", "3*nmeshvert"),
]


# appended to struct mjh_model in round 2 (behind the name tables): sites, sensors, mocap bodies
_INT_SIZES2 = ["nsite", "nsensor", "nsensordata", "nmocap"]
_ARRAYS2 = [
    ("site_bodyid", "i", "nsite"), ("site_pos", "d", "3*nsite"), ("site_quat", "d", "4*nsite"),
    ("sensor_type", "i", "nsensor"), ("sensor_objid", "i", "nsensor"), ("sensor_adr", "i", "nsensor"),
]
_ARRAYS3 = [("body_mocapid", "i", "nbody")]
# appended for height fields (behind body_mocapid)
_INT_SIZES4 = ["nhfield", "nhfielddata"]
_ARRAYS4 = [
    ("hfield_nrow", "i", "nhfield"), ("hfield_ncol", "i", "nhfield"), ("hfield_adr", "i", "nhfield"),
    ("hfield_size", "d", "4*nhfield"), ("hfield_data", "d", "nhfielddata"),
]
# appended for ray casting against mesh geoms (behind hfield_names): the hull planes of the kept vertices
_INT_SIZES5 = ["nmeshplane"]
_ARRAYS5 = [("mesh_planeadr", "i", "nmesh"), ("mesh_planenum", "i", "nmesh"), ("mesh_plane", "d", "4*nmeshplane")]
# appended for depth cameras (behind mesh_plane)
_INT_SIZES6 = ["ncam"]
_ARRAYS6 = [("cam_bodyid", "i", "ncam"), ("cam_pos", "d", "3*ncam"), ("cam_quat", "d", "4*ncam"), ("cam_fovy", "d", "ncam")]
# appended for rays against a mesh's own triangles (behind cam_names)
_INT_SIZES7 = ["nmeshtri"]
_ARRAYS7 = [("mesh_triadr", "i", "nmesh"), ("mesh_trinum", "i", "nmesh"), ("mesh_tri", "d", "9*nmeshtri")]
# appended for colour images (behind mesh_tri)
_ARRAYS8 = [("geom_rgba", "d", "4*ngeom")]
# appended for lights (behind geom_rgba)
_INT_SIZES9 = ["nlight"]
_ARRAYS9 = [
    ("light_bodyid", "i", "nlight"), ("light_pos", "d", "3*nlight"), ("light_dir", "d", "3*nlight"),
    ("light_directional", "i", "nlight"), ("light_castshadow", "i", "nlight"), ("light_active", "i", "nlight"),
    ("light_diffuse", "d", "3*nlight"), ("light_ambient", "d", "3*nlight"), ("light_cutoff", "d", "nlight"),
    ("light_exponent", "d", "nlight"),
]
MAXLIGHT = 8   # MJH_MAXLIGHT
# appended for textures (behind light_names); "B": unsigned char
_INT_SIZES10 = ["ntex", "ntexdata"]
_ARRAYS10 = [("tex_width", "i", "ntex"), ("tex_height", "i", "ntex"), ("tex_adr", "i", "ntex"), ("tex_rgb", "B", "3*ntexdata")]
_ARRAYS10B = [("geom_texid", "i", "ngeom"), ("geom_texrepeat", "d", "2*ngeom"), ("geom_texuniform", "i", "ngeom")]
c_ubyte_p = C.POINTER(C.c_ubyte)
_PTR = {"i": c_int_p, "d": c_double_p, "B": c_ubyte_p}
MAXTEXSIZE, MAXTEXDATA = 4096, 1 << 24   # MJH_MAXTEXSIZE, MJH_MAXTEXDATA
TEXBUILTIN = {"flat": 0, "checker": 1, "gradient": 2}   # enum mjh_texbuiltin
TEXMARK = {"none": 0, "edge": 1, "cross": 2}            # enum mjh_texmark


class Model(C.Structure):
    _fields_ = (
        [(n, C.c_int) for n in _INT_SIZES]
        + [("opt", Option), ("meaninertia", C.c_double)]
        + [(n, c_int_p if t == "i" else c_double_p) for n, t, _ in _ARRAYS]
        + [("body_names", C.POINTER(C.c_char_p)), ("jnt_names", C.POINTER(C.c_char_p)),
           ("geom_names", C.POINTER(C.c_char_p))]
        + [(n, C.c_int) for n in _INT_SIZES2]
        + [(n, c_int_p if t == "i" else c_double_p) for n, t, _ in _ARRAYS2]
        + [("site_names", C.POINTER(C.c_char_p)), ("sensor_names", C.POINTER(C.c_char_p))]
        + [(n, c_int_p if t == "i" else c_double_p) for n, t, _ in _ARRAYS3]
        + [(n, C.c_int) for n in _INT_SIZES4]
        + [(n, c_int_p if t == "i" else c_double_p) for n, t, _ in _ARRAYS4]
        + [("hfield_names", C.POINTER(C.c_char_p))]
        + [(n, C.c_int) for n in _INT_SIZES5]
        + [(n, c_int_p if t == "i" else c_double_p) for n, t, _ in _ARRAYS5]
        + [(n, C.c_int) for n in _INT_SIZES6]
        + [(n, c_int_p if t == "i" else c_double_p) for n, t, _ in _ARRAYS6]
        + [("cam_names", C.POINTER(C.c_char_p))]
        + [(n, C.c_int) for n in _INT_SIZES7]
        + [(n, c_int_p if t == "i" else c_double_p) for n, t, _ in _ARRAYS7]
        + [(n, c_int_p if t == "i" else c_double_p) for n, t, _ in _ARRAYS8]
        + [(n, C.c_int) for n in _INT_SIZES9]
        + [(n, c_int_p if t == "i" else c_double_p) for n, t, _ in _ARRAYS9]
        + [("light_names", C.POINTER(C.c_char_p))]
        + [(n, C.c_int) for n in _INT_SIZES10]
        + [(n, _PTR[t]) for n, t, _ in _ARRAYS10]
        + [("tex_names", C.POINTER(C.c_char_p))]
        + [(n, _PTR[t]) for n, t, _ in _ARRAYS10B]
    )

    def array(self, name):
        """numpy copy of a model array."""
        import numpy as np

        for n, t, expr in _ARRAYS + _ARRAYS2 + _ARRAYS3 + _ARRAYS4 + _ARRAYS5 + _ARRAYS6 + _ARRAYS7 + _ARRAYS8 + _ARRAYS9 + _ARRAYS10 + _ARRAYS10B:
            if n == name:
                ln = eval(expr, {}, {k: getattr(self, k) for k in _INT_SIZES + _INT_SIZES2 + _INT_SIZES4 + _INT_SIZES5 + _INT_SIZES6 + _INT_SIZES7 + _INT_SIZES9 + _INT_SIZES10})
                ptr = getattr(self, n)
                if ln == 0 or not ptr:
                    return np.zeros(0, dtype={"i": np.int32, "d": np.float64, "B": np.uint8}[t])
                return np.ctypeslib.as_array(ptr, shape=(ln,)).copy()
        raise KeyError(name)


Model_p = C.POINTER(Model)

class LoadOptions(C.Structure):
    _fields_ = [("boundmass", C.c_double), ("boundinertia", C.c_double), ("robot_gravcomp", C.c_int), ("load_meshes", C.c_int),
                ("odom_joints", C.c_uint), ("nrobot_pose", C.c_int), ("robot_pose_body", C.POINTER(C.c_char_p)), ("robot_pose", c_double_p), ("parent_child_exclude", C.c_int)]


class RayOptions(C.Structure):
    _fields_ = [("site", C.c_int), ("bodyexclude", C.c_int), ("flg_static", C.c_int), ("per_env", C.c_int), ("cutoff", C.c_double)]

class DepthOptions(C.Structure):
    _fields_ = [("camera", C.c_int), ("width", C.c_int), ("height", C.c_int), ("bodyexclude", C.c_int), ("flg_static", C.c_int),
                ("range", C.c_int), ("cull", C.c_int), ("cutoff", C.c_double)]

class ScanOptions(C.Structure):
    _fields_ = [("site", C.c_int), ("width", C.c_int), ("height", C.c_int), ("azimuth0", C.c_double), ("azimuth_step", C.c_double),
                ("elevation", c_double_p), ("elevation0", C.c_double), ("elevation_step", C.c_double), ("bodyexclude", C.c_int),
                ("flg_static", C.c_int), ("cull", C.c_int), ("cutoff", C.c_double)]

class HeightScanOptions(C.Structure):
    _fields_ = [("site", C.c_int), ("align", C.c_int), ("width", C.c_int), ("height", C.c_int), ("spacing", C.c_double * 2),
                ("offset", C.c_double * 2), ("above", C.c_double), ("bodyexclude", C.c_int), ("exclude_tree", C.c_int),
                ("flg_static", C.c_int), ("cull", C.c_int), ("cutoff", C.c_double)]

class Frame(C.Structure):
    _fields_ = [("objtype", C.c_int), ("id", C.c_int), ("reftype", C.c_int), ("refid", C.c_int), ("flags", C.c_int)]

MJH_FRAME_LOCAL, MJH_FRAME_PROPER = 1, 2   # mjh_frame.flags (PROPER: mjh_frame_accel only)

class LightOptions(C.Structure):
    _fields_ = [("shadows", C.c_int), ("cull", C.c_int), ("bias", C.c_float)]

class RenderOptions(C.Structure):
    _fields_ = [("view", DepthOptions), ("ambient", C.c_float), ("diffuse", C.c_float), ("background", C.c_float * 4)]


# every symbol include/mjhip.h declares: (name, restype, argtypes)
_vp = C.c_void_p
SYMBOLS = [
    ("mjh_builder_create", _vp, []),
    ("mjh_builder_destroy", None, [_vp]),
    ("mjh_builder_set_option", None, [_vp, C.POINTER(Option)]),
    ("mjh_builder_get_option", None, [_vp, C.POINTER(Option)]),
    ("mjh_builder_set_capacity", None, [_vp, C.c_int, C.c_int]),
    ("mjh_builder_set_bounds", None, [_vp, C.c_double, C.c_double]),
    ("mjh_builder_set_balanceinertia", None, [_vp, C.c_int]),
    ("mjh_builder_add_body", C.c_int, [_vp, C.c_char_p, C.c_int, c_double_p, c_double_p, C.c_double]),
    ("mjh_builder_set_inertial", C.c_int, [_vp, C.c_int, C.c_double, c_double_p, c_double_p, c_double_p]),
    ("mjh_builder_add_joint", C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p,
                                       C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    ("mjh_builder_add_geom", C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p,
                                      c_double_p, C.c_int, C.c_int, C.c_int, C.c_double]),
    ("mjh_builder_add_mesh", C.c_int, [_vp, c_double_p, C.c_int, c_int_p, C.c_int, c_double_p]),
    ("mjh_builder_add_mesh_stl", C.c_int, [_vp, C.c_char_p, c_double_p]),
    ("mjh_builder_add_hfield", C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, c_double_p, c_double_p]),
    ("mjh_builder_add_hfield_geom", C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p,
                                             C.c_int, C.c_int, C.c_int]),
    ("mjh_builder_add_mesh_geom", C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p,
                                           C.c_int, C.c_int, C.c_int, C.c_double]),
    ("mjh_builder_add_exclude", C.c_int, [_vp, C.c_int, C.c_int]),
    ("mjh_builder_add_eq_joint", C.c_int, [_vp, C.c_int, C.c_int, c_double_p]),
    ("mjh_builder_add_eq_connect", C.c_int, [_vp, C.c_int, C.c_int, c_double_p]),
    ("mjh_builder_add_eq_weld", C.c_int, [_vp, C.c_int, C.c_int, c_double_p, C.c_double]),
    ("mjh_builder_set_mocap", C.c_int, [_vp, C.c_int]),
    ("mjh_builder_add_site", C.c_int, [_vp, C.c_char_p, C.c_int, c_double_p, c_double_p]),
    ("mjh_builder_add_camera", C.c_int, [_vp, C.c_char_p, C.c_int, c_double_p, c_double_p, C.c_double]),
    ("mjh_builder_set_geom_rgba", C.c_int, [_vp, C.c_int, c_double_p]),
    ("mjh_builder_add_light", C.c_int, [_vp, C.c_char_p, C.c_int, c_double_p, c_double_p, C.c_int, C.c_int, c_double_p, c_double_p,
                                       C.c_double, C.c_double]),
    ("mjh_builder_set_light_active", C.c_int, [_vp, C.c_int, C.c_int]),
    ("mjh_builder_add_texture", C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, c_ubyte_p]),
    ("mjh_builder_add_texture_builtin", C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p]),
    ("mjh_builder_set_geom_texture", C.c_int, [_vp, C.c_int, C.c_int, c_double_p, C.c_int]),
    ("mjh_builder_add_sensor", C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int]),
    ("mjh_builder_compile", Model_p, [_vp]),
    ("mjh_model_destroy", None, [Model_p]),
    ("mjh_model_replicate", Model_p, [Model_p, C.c_int]),
    ("mjh_name2id", C.c_int, [Model_p, C.c_int, C.c_char_p]),
    ("mjh_id2name", C.c_char_p, [Model_p, C.c_int, C.c_int]),
    ("mjh_load_mjcf_string", Model_p, [C.c_char_p]),
    ("mjh_load_mjcf_file", Model_p, [C.c_char_p]),
    ("mjh_load_mjcf_files", Model_p, [C.POINTER(C.c_char_p), C.c_int]),
    ("mjh_load_note", C.c_char_p, []),
    ("mjh_load_default_options", None, [C.POINTER(LoadOptions)]),
    ("mjh_load_mjcf_files_opt", Model_p, [C.POINTER(C.c_char_p), C.c_int, C.POINTER(LoadOptions)]),
    ("mjh_load_set_bounds", None, [C.c_double, C.c_double]),
    ("mjh_load_set_mesh_mode", None, [C.c_int]),
    ("mjh_load_set_textures", None, [C.c_int]),
    ("mjh_load_set_robot_gravcomp", None, [C.c_int]),
    ("mjh_load_set_odom_joints", None, [C.c_uint]),
    ("mjh_load_set_parent_child_exclude", None, [C.c_int]),
    ("mjh_load_set_robot_pose", None, [C.c_char_p, c_double_p]),
    ("mjh_scene_s24", Model_p, []),
    ("mjh_scene_s24_pen", Model_p, [C.c_double, C.c_int]),
    ("mjh_scene_s24_randomize", C.c_int, [Model_p, C.c_int, C.c_int, C.c_uint] + [c_double_p] * 7),
    ("mjh_scene_boxes_randomize", C.c_int, [Model_p, C.c_int, C.c_int, C.c_uint, C.c_double] + [c_double_p] * 7),
    ("mjh_scene_pendulum", Model_p, []),
    ("mjh_scene_arm7", Model_p, [C.c_int]),
    ("mjh_scene_boxpile", Model_p, [C.c_int]),
    ("mjh_create", C.c_int, [Model_p, C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    ("mjh_destroy", None, [_vp]),
    ("mjh_step1", C.c_int, [_vp]),
    ("mjh_step2", C.c_int, [_vp]),
    ("mjh_step", C.c_int, [_vp, C.c_int, C.c_int]),
    ("mjh_inverse", C.c_int, [_vp]),
    ("mjh_forward", C.c_int, [_vp]),
    ("mjh_mulM", C.c_int, [_vp, C.c_int, C.c_int, c_double_p, c_double_p]),
    ("mjh_synchronize", C.c_int, [_vp]),
    ("mjh_set_cmd", C.c_int, [_vp, C.c_int, C.c_int, c_double_p, c_double_p]),
    ("mjh_set_pd_controller", C.c_int, [_vp, C.c_double, C.c_double]),
    ("mjh_set_pd_target", C.c_int, [_vp, C.c_int, C.c_int, c_double_p]),
    ("mjh_set_controlled_dofs", C.c_int, [_vp, c_int_p]),
    ("mjh_set_odom_dofs", C.c_int, [_vp, c_int_p, c_int_p, c_int_p]),
    ("mjh_set_odom_vel", C.c_int, [_vp, C.c_int, C.c_int, c_double_p]),
    ("mjh_get_joint_state", C.c_int, [_vp, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p]),
    ("mjh_get_body_state", C.c_int, [_vp, C.c_int, C.c_int, c_double_p, c_double_p]),
    ("mjh_get_geom_state", C.c_int, [_vp, C.c_int, C.c_int, c_double_p, c_double_p]),
    ("mjh_get_state", C.c_int, [_vp, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]),
    ("mjh_set_state", C.c_int, [_vp, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]),
    ("mjh_get_field", C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, c_double_p]),
    ("mjh_get_stats", C.c_int, [_vp, C.c_int, C.c_int, c_int_p]),
    ("mjh_get_contacts", C.c_int, [_vp, C.c_int, c_double_p, c_double_p, c_double_p, c_int_p]),
    ("mjh_set_xfrc_applied", C.c_int, [_vp, C.c_int, C.c_int, c_double_p]),
    ("mjh_get_xfrc_applied", C.c_int, [_vp, C.c_int, C.c_int, c_double_p]),
    ("mjh_get_sensordata", C.c_int, [_vp, C.c_int, C.c_int, c_double_p]),
    ("mjh_set_mocap_pose", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, c_double_p, c_double_p]),
    ("mjh_set_env_param", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, c_double_p]),
    ("mjh_transplant_state", C.c_int, [_vp, _vp, C.c_int]),
    ("mjh_set_initial_qpos", C.c_int, [_vp, C.c_int, C.c_int, c_double_p]),
    ("mjh_reset", C.c_int, [_vp, c_int_p, C.c_int]),
    ("mjh_set_slot_active", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("mjh_set_body_pose", C.c_int, [_vp, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p]),
    ("mjh_spawn_objects", C.c_int, [_vp, C.c_int, c_int_p, c_int_p, c_double_p, c_double_p, c_double_p]),
    ("mjh_destroy_objects", C.c_int, [_vp, C.c_int, c_int_p, c_int_p]),
    ("mjh_ray_default_options", None, [C.POINTER(RayOptions)]),
    ("mjh_ray", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, c_double_p, c_double_p, C.POINTER(RayOptions), c_double_p, c_int_p]),
    ("mjh_ray_device", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.POINTER(RayOptions), _vp, _vp]),
    ("mjh_ray_skipped_geoms", C.c_int, [Model_p]),
    ("mjh_ray_set_mesh_mode", C.c_int, [_vp, C.c_int]),
    ("mjh_ray_get_mesh_mode", C.c_int, [_vp]),
    ("mjh_ray_set_mesh_surface", C.c_int, [_vp, C.c_int]),
    ("mjh_ray_get_mesh_surface", C.c_int, [_vp]),
    ("mjh_depth_default_options", None, [C.POINTER(DepthOptions)]),
    ("mjh_depth", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(DepthOptions), _vp, _vp]),
    ("mjh_depth_device", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(DepthOptions), _vp, _vp]),
    ("mjh_scan_default_options", None, [C.POINTER(ScanOptions)]),
    ("mjh_scan", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(ScanOptions), _vp, _vp, _vp]),
    ("mjh_scan_device", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(ScanOptions), _vp, _vp, _vp]),
    ("mjh_heightscan_default_options", None, [C.POINTER(HeightScanOptions)]),
    ("mjh_heightscan", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(HeightScanOptions), _vp, _vp, _vp]),
    ("mjh_heightscan_device", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(HeightScanOptions), _vp, _vp, _vp]),
    ("mjh_render_default_options", None, [C.POINTER(RenderOptions)]),
    ("mjh_render", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(RenderOptions), _vp, _vp, _vp, _vp]),
    ("mjh_render_device", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(RenderOptions), _vp, _vp, _vp, _vp]),
    ("mjh_light_default_options", None, [C.POINTER(LightOptions)]),
    ("mjh_render_set_lighting", C.c_int, [_vp, C.c_int]),
    ("mjh_render_get_lighting", C.c_int, [_vp]),
    ("mjh_render_set_light_options", C.c_int, [_vp, C.POINTER(LightOptions)]),
    ("mjh_render_get_light_options", C.c_int, [_vp, C.POINTER(LightOptions)]),
    ("mjh_set_light_active", C.c_int, [_vp, C.c_int, C.c_int]),
    ("mjh_render_set_texturing", C.c_int, [_vp, C.c_int]),
    ("mjh_render_get_texturing", C.c_int, [_vp]),
    ("mjh_export_state_device", C.c_int, [_vp, _vp]),
    ("mjh_state_stride", C.c_int, [_vp]),
    ("mjh_mirror_create", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    ("mjh_mirror_destroy", None, [_vp]),
    ("mjh_mirror_update", C.c_int, [_vp, C.c_int]),
    ("mjh_mirror_wait", C.c_int, [_vp]),
    ("mjh_mirror_field", C.POINTER(C.c_float), [_vp, C.c_int, C.POINTER(C.c_int)]),
    ("mjh_mirror_time", c_double_p, [_vp]),
    ("mjh_debug_stage_cycles", C.c_int, [_vp, C.c_int, c_double_p]),
    ("mjh_debug_stage_raw", C.c_int, [_vp, C.c_int, _vp]),
    ("mjh_debug_solve_probe", C.c_int, [_vp, C.c_int, C.c_int, c_double_p, c_double_p]),
    ("mjh_debug_stop_at", C.c_int, [_vp, C.c_int, C.c_int]),
    ("mjh_set_timestep", C.c_int, [_vp, C.c_double]),
    ("mjh_get_timestep", C.c_double, [_vp]),
    ("mjh_set_layout_policy", None, [C.c_int]),
    ("mjh_set_window_solver", None, [C.c_int]),
    ("mjh_window_solver", C.c_int, [_vp]),
    ("mjh_set_contact_report", None, [C.c_int]),
    ("mjh_contact_report", C.c_int, [_vp]),
    ("mjh_contact_report_device", C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_int_p]),
    ("mjh_get_contact_forces", C.c_int, [_vp, C.c_int, C.c_int, c_int_p, c_double_p, c_double_p, c_double_p, c_double_p, c_int_p, c_int_p]),
    ("mjh_get_cfrc_ext", C.c_int, [_vp, C.c_int, C.c_int, c_double_p]),
    ("mjh_body_contact_force_device", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, _vp, _vp]),
    ("mjh_body_contact_force", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, c_double_p, c_int_p]),
    ("mjh_frame_state_device", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    ("mjh_frame_state", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, c_double_p, c_double_p]),
    ("mjh_frame_accel_device", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    ("mjh_frame_accel", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, c_double_p, c_double_p]),
    ("mjh_set_cmd_device", C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    ("mjh_set_pd_target_device", C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    ("mjh_set_xfrc_applied_device", C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    ("mjh_get_joint_state_device", C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    ("mjh_reset_device", C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    ("mjh_set_pgs_row_order", None, [C.c_int]),
    ("mjh_set_cohorts", C.c_int, [_vp, C.c_int]),
    ("mjh_get_cohorts", C.c_int, [_vp]),
    ("mjh_set_steps_per_launch", C.c_int, [_vp, C.c_int]),
    ("mjh_get_steps_per_launch", C.c_int, [_vp]),
    ("mjh_set_chain_graph", None, [C.c_int]),
    ("mjh_launches_per_step", C.c_int, [C.c_void_p]),
    ("mjh_set_launch_timing", C.c_int, [_vp, C.c_int]),
    ("mjh_get_launch_timing", C.c_int, [_vp, c_double_p, C.POINTER(C.c_int)]),
    ("mjh_group_create", C.c_int, [Model_p, C.c_int, c_int_p, C.c_int, C.POINTER(_vp)]),
    ("mjh_group_destroy", None, [_vp]),
    ("mjh_group_ndev", C.c_int, [_vp]),
    ("mjh_group_nenv", C.c_int, [_vp]),
    ("mjh_group_engine", _vp, [_vp, C.c_int]),
    ("mjh_group_env_range", C.c_int, [_vp, C.c_int, c_int_p, c_int_p]),
    ("mjh_group_locate", C.c_int, [_vp, C.c_int, c_int_p, c_int_p]),
    ("mjh_group_step", C.c_int, [_vp, C.c_int, C.c_int]),
    ("mjh_group_step1", C.c_int, [_vp]),
    ("mjh_group_inverse", C.c_int, [_vp]),
    ("mjh_group_step2", C.c_int, [_vp]),
    ("mjh_group_reset", C.c_int, [_vp]),
    ("mjh_group_synchronize", C.c_int, [_vp]),
    ("mjh_group_publish", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("mjh_group_state_device", C.POINTER(C.c_float), [_vp, C.c_int]),
    ("mjh_group_state_stride", C.c_int, [_vp]),
    ("mjh_group_uses_rccl", C.c_int, [_vp]),
    ("mjh_group_set_transport", None, [C.c_int]),
    ("mjh_debug_rccl_exchange", C.c_int, [C.c_int, C.c_int, C.c_ulong, C.c_int]),
    ("mjh_group_set_host_threads", None, [C.c_int]),
    ("mjh_group_host_threads", C.c_int, [C.c_void_p]),
    ("mjh_group_wait_publish", C.c_int, [_vp, C.c_int, _vp]),
    ("mjh_group_release_publish", C.c_int, [_vp, C.c_int, _vp]),
    ("mjh_group_set_publish_timing", C.c_int, [_vp, C.c_int]),
    ("mjh_group_get_publish_timing", C.c_int, [_vp, c_double_p, C.POINTER(C.c_int)]),
    ("mjh_nenv", C.c_int, [_vp]),
    ("mjh_engine_model", Model_p, [_vp]),
    ("mjh_lds_bytes", C.c_int, [_vp]),
    ("mjh_solver_order", C.c_int, [_vp]),
    ("mjh_pgs_schedule", C.c_int, [_vp]),
    ("mjh_patch_sweep", C.c_int, [_vp]),
    ("mjh_dense_solver", C.c_int, [_vp]),
    ("mjh_query_lds_bytes", C.c_int, [Model_p]),
    ("mjh_query_lds_bytes_assemble", C.c_int, [Model_p]),
    ("mjh_debug_lds_layout", C.c_int, [Model_p, C.c_char_p, C.c_int]),
    ("mjh_host_run_pd", C.c_int, [_vp, C.c_int, c_double_p, C.c_double, C.c_double, C.c_long, c_double_p, c_double_p, c_double_p]),
    ("mjh_host_run_pd_group", C.c_int, [_vp, C.c_int, c_double_p, C.c_double, C.c_double, C.c_long, C.c_int, c_double_p, c_double_p, C.POINTER(C.c_float)]),
    ("mjh_host_run_realtime", C.c_int, [_vp, C.c_int, c_double_p, C.c_double, C.c_double, C.c_long, C.c_double, c_double_p]),
    ("mjh_last_error", C.c_char_p, []),
    ("mjh_version", C.c_char_p, []),
]

_lib = None


def load(path=None, strict=True):
    """Load libmjhip.so and attach prototypes.  Raises if the library is absent
    (no fallback: the HIP extension IS the product)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
    for name, res, args in SYMBOLS:
        if not strict and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def dptr(a):
    """double* of a contiguous float64 numpy array (or None)."""
    if a is None:
        return None
    return a.ctypes.data_as(c_double_p)


def iptr(a):
    if a is None:
        return None
    return a.ctypes.data_as(c_int_p)
