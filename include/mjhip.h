/* mjhip.h — C ABI of the MI355X-native many-environment rigid-body stepper.
 *
 * This is the drop-in boundary for the hot path of HoangGiang93/mujoco_sim: the
 * reference has no plugin interface; its boundary IS the handful of MuJoCo C
 * calls made by the step driver plus the raw mjModel/mjData fields the wrapper
 * dereferences.  Every entry point below names the reference
 * call site (file:line under /root/reference) it replaces.
 *
 * Conventions
 *   - plain C linkage, plain pointers and sizes, no exceptions across the ABI
 *   - return 0 on success, negative mjh_error on failure; text in mjh_last_error()
 *   - host I/O is double (mjtNum / ros_control handles are double,
 *     include/mujoco_sim/mj_hw_interface.h:58-65); device arithmetic is fp32
 *   - one stepping thread per engine (the reference serialises on `mtx`,
 *     src/mj_main.cpp:82,112)
 *   - "env" = one independent copy of the simulated world (the reference has
 *     exactly one: the globals `m`,`d`, include/mujoco_sim/mj_model.h:29-30)
 */
#ifndef MJHIP_H_
#define MJHIP_H_

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ enums */

enum mjh_error {
  MJH_OK = 0,
  MJH_ERR_ARG = -1,        /* bad argument / index out of range            */
  MJH_ERR_NO_DEVICE = -2,  /* no HIP device / HIP runtime failure          */
  MJH_ERR_CAPACITY = -3,   /* model exceeds what the kernels support       */
  MJH_ERR_STATE = -4,      /* call sequence violation (step2 before step1) */
  MJH_ERR_UNSUPPORTED = -5 /* feature not implemented                      */
};

/* joint types: values follow MuJoCo's mjtJoint so that jnt_type tables read by
 * the wrapper (mj_sim.cpp:503-513, mj_ros.cpp:2164-2194) keep their meaning */
enum mjh_joint { MJH_JNT_FREE = 0, MJH_JNT_BALL = 1, MJH_JNT_SLIDE = 2, MJH_JNT_HINGE = 3 };

/* geom types: values follow mjtGeom (read by mj_ros.cpp:1968-2094) */
enum mjh_geom {
  MJH_GEOM_PLANE = 0, MJH_GEOM_HFIELD = 1, MJH_GEOM_SPHERE = 2, MJH_GEOM_CAPSULE = 3,
  MJH_GEOM_ELLIPSOID = 4, MJH_GEOM_CYLINDER = 5, MJH_GEOM_BOX = 6, MJH_GEOM_MESH = 7
};

/* contacts one (hfield, geom) pair can produce: the first ones in prism order are kept (MuJoCo's mjMAXCONPAIR) */
#define MJH_HFIELD_MAXCON 50

enum mjh_eq { MJH_EQ_CONNECT = 0, MJH_EQ_WELD = 1, MJH_EQ_JOINT = 2 };
/* sensor types: values follow mjtSensor; the reference publishes exactly these two (MjSim::init_sensors, mj_sim.cpp:973-1014) */
enum mjh_sensor { MJH_SENS_FORCE = 4, MJH_SENS_TORQUE = 5 };

/* constraint row types (order of assembly: equality, friction loss, limit, contact) */
enum mjh_cnstr {
  MJH_CNSTR_EQUALITY = 0, MJH_CNSTR_FRICTION_DOF = 1, MJH_CNSTR_LIMIT_JOINT = 3,
  MJH_CNSTR_CONTACT_FRICTIONLESS = 5, MJH_CNSTR_CONTACT_PYRAMIDAL = 6
};

/* disable-flag bits (subset of mjtDisableBit that this path honours) */
enum mjh_disable {
  MJH_DSBL_CONSTRAINT = 1 << 0, MJH_DSBL_EQUALITY = 1 << 1, MJH_DSBL_FRICTIONLOSS = 1 << 2,
  MJH_DSBL_LIMIT = 1 << 3, MJH_DSBL_CONTACT = 1 << 4, MJH_DSBL_PASSIVE = 1 << 5,
  MJH_DSBL_GRAVITY = 1 << 6, MJH_DSBL_WARMSTART = 1 << 8, MJH_DSBL_FILTERPARENT = 1 << 9,
  MJH_DSBL_REFSAFE = 1 << 11, MJH_DSBL_EULERDAMP = 1 << 13
};

/* per-env parameter tables that may override the shared model (S24 draws box
 * half-extents per env) */
enum mjh_env_param {
  MJH_EP_GEOM_SIZE = 0,       /* 3*ngeom  */
  MJH_EP_GEOM_RBOUND = 1,     /* ngeom    */
  MJH_EP_BODY_MASS = 2,       /* nbody    */
  MJH_EP_BODY_INERTIA = 3,    /* 3*nbody  */
  MJH_EP_BODY_INVWEIGHT0 = 4, /* 2*nbody  */
  MJH_EP_DOF_INVWEIGHT0 = 5,  /* nv       */
  MJH_EP_COUNT = 6
};

/* ------------------------------------------------------------ model (IR) */

typedef struct mjh_option {
  double timestep;          /* model/world/empty.xml:2 -> 0.005                */
  double gravity[3];
  int iterations;           /* main solver sweeps (MuJoCo default 100)         */
  double tolerance;         /* scaled-improvement threshold (default 1e-8)     */
  double impratio;          /* default 1                                       */
  int noslip_iterations;    /* model/ontology/scene.xml:2-3; 0 = off (default)  */
  int disableflags;         /* mjh_disable bits                                */
  double noslip_tolerance;  /* model/ontology/scene.xml:3 (MuJoCo default 1e-6) */
} mjh_option;

/* Compiled, topology-sorted model: the subset of mjModel this path reads
 * (SURVEY.md §8-b B1 lists the fields the wrapper itself touches).  All arrays
 * are owned by the model object; bodies are sorted parents-first, body 0 is
 * the world. */
typedef struct mjh_model {
  /* sizes */
  int nq, nv, nbody, njnt, ngeom, neq, npair, nM, ntree, nexclude;
  int maxcon;  /* contact capacity per env (contacts beyond it are dropped + flagged) */
  int maxefc;  /* constraint-row capacity per env                                     */
  int nmesh, nmeshvert; /* convex mesh assets: count, total vertices                    */
  mjh_option opt;
  double meaninertia; /* stat.meaninertia: mean diag(M(qpos0)) — scales solver tolerance */

  /* bodies */
  int *body_parentid, *body_rootid, *body_weldid, *body_jntadr, *body_jntnum;
  int *body_dofadr, *body_dofnum, *body_treeid, *body_level, *body_geomadr, *body_geomnum;
  double *body_pos, *body_quat, *body_ipos, *body_iquat, *body_mass, *body_inertia;
  double *body_gravcomp, *body_invweight0; /* [2*nbody] translational, rotational */
  /* joints */
  int *jnt_type, *jnt_qposadr, *jnt_dofadr, *jnt_bodyid, *jnt_limited;
  double *jnt_pos, *jnt_axis, *jnt_stiffness, *jnt_range, *jnt_margin;
  double *jnt_solref, *jnt_solimp; /* [2*njnt], [5*njnt] limit parameters */
  double *qpos0, *qpos_spring;
  /* dofs */
  int *dof_bodyid, *dof_jntid, *dof_parentid, *dof_Madr, *dof_treeid;
  double *dof_armature, *dof_damping, *dof_frictionloss, *dof_invweight0;
  double *dof_solref, *dof_solimp; /* friction-loss parameters */
  /* trees (a tree = a child of the world with all its descendants; contiguous dofs) */
  int *tree_dofadr, *tree_dofnum, *tree_bodyid;
  /* geoms */
  int *geom_type, *geom_bodyid, *geom_condim, *geom_contype, *geom_conaffinity, *geom_priority;
  double *geom_pos, *geom_quat, *geom_size, *geom_rbound, *geom_friction;
  double *geom_solmix, *geom_solref, *geom_solimp, *geom_margin, *geom_gap;
  /* static candidate pair list: geom1 < geom2 by (type, then id) ordering rule of
   * the narrow phase; filters (same/weld body, parent-child, contype/conaffinity,
   * <exclude>) applied at compile time */
  int *pair_geom1, *pair_geom2;
  /* equality constraints */
  int *eq_type, *eq_obj1id, *eq_obj2id, *eq_active;
  double *eq_data, *eq_solref, *eq_solimp; /* [11*neq], [2*neq], [5*neq] */
  /* convex mesh assets (mjModel mesh_vert / geom_dataid; pr2.xml:5-22): the support-relevant vertices of each
   * mesh in the mesh geom's own frame (origin = centre of mass, axes = principal axes) */
  int *geom_dataid;                /* [ngeom] mesh id of a mesh geom, -1 otherwise */
  int *mesh_vertadr, *mesh_vertnum; /* [nmesh] */
  double *mesh_vert;                /* [3*nmeshvert] */
  /* name tables: resolved ONCE on the host (the reference calls mj_name2id per
   * joint per step: mj_hw_interface.cpp:64,79; mj_sim.cpp:1060,1083-1146) */
  char **body_names, **jnt_names, **geom_names;
  /* ---- appended in round 2 (older fields keep their offsets) ----
   * sites and force / torque sensors (m->nsensor, sensor_type, sensor_objid, sensor_adr, nsensordata: mj_sim.cpp:973-1014,
   * mj_ros.cpp:1933-1966); a sensor measures the interaction force (torque) between its site's body and that body's parent,
   * in the site frame, 3 numbers each */
  int nsite, nsensor, nsensordata, nmocap;
  int* site_bodyid; double *site_pos, *site_quat;      /* [nsite], [3*nsite], [4*nsite]: site frame in its body */
  int *sensor_type, *sensor_objid, *sensor_adr;        /* [nsensor]: mjh_sensor, site id, first index in sensordata */
  char **site_names, **sensor_names;
  /* mocap bodies (the `_ref` bodies MjSim::init_references welds robot links to, mj_sim.cpp:847-960): static children of the
   * world whose pose is an INPUT per environment (mjh_set_mocap_pose); body_mocapid[b] = index or -1; their initial pose is
   * body_pos / body_quat.  eq_type CONNECT / WELD: eq_obj1id / eq_obj2id are BODY ids (0 = world) and eq_data holds
   *   connect: [0..2] anchor in body1's frame, [3..5] the same point in body2's frame at qpos0
   *   weld:    [0..2] anchor in body2's frame, [3..5] the same point in body1's frame at qpos0,
   *            [6..9] relative orientation quat(body2)^-1 * quat(body1) at qpos0, [10] torquescale */
  int* body_mocapid;
  /* ---- appended for height fields (older fields keep their offsets) ----
   * <asset><hfield>: an nrow x ncol elevation grid, row-major, normalised to [0, 1] at compile time.  Grid point (r, c) lies at
   * x = -size[0] + 2 size[0] c / (ncol - 1), y = -size[1] + 2 size[1] r / (nrow - 1), z = data size[2] in the geom's frame; the
   * terrain reaches down to z = -size[3].  geom_dataid of an hfield geom holds its hfield id. */
  int nhfield, nhfielddata;
  int *hfield_nrow, *hfield_ncol, *hfield_adr;  /* [nhfield] */
  double* hfield_size;                          /* [4*nhfield]: radius_x, radius_y, elevation_z, base_z */
  double* hfield_data;                          /* [nhfielddata] */
  char** hfield_names;
  /* ---- appended for ray casting against mesh geoms (older fields keep their offsets) ----
   * the facets of the convex hull of each mesh's kept vertices (exactly the points of mesh_vert, so a ray sees the solid the narrow
   * phase collides), coplanar facets merged: every distinct plane once.  A mesh whose kept vertices span no volume has
   * mesh_planenum 0 (no ray sees it). */
  int nmeshplane;
  int *mesh_planeadr, *mesh_planenum;   /* [nmesh] */
  double* mesh_plane;                   /* [4*nmeshplane]: unit outward normal n, offset d; inside is n.x <= d;
                                           frame of mesh_vert (the mesh geom's own frame) */
  /* ---- appended for depth cameras (older fields keep their offsets) ----
   * <camera mode="fixed">: a frame attached to a body; MuJoCo's convention: the camera looks along its -z, +x is right, +y is up.
   * mjh_depth renders from it (below); resolution, sensor attributes, near planes and the other modes are not modelled. */
  int ncam;
  int* cam_bodyid;              /* [ncam] */
  double *cam_pos, *cam_quat;   /* [3 ncam], [4 ncam]: camera frame in its body */
  double* cam_fovy;             /* [ncam] vertical field of view, degrees */
  char** cam_names;
  /* ---- appended for rays against a mesh's own triangles (older fields keep their offsets) ----
   * the triangles of the mesh file (or of mjh_builder_add_mesh's face list) as coordinates, moved into the frame of mesh_vert with
   * the vertices and taken BEFORE those are de-duplicated and thinned; a triangle without area (two equal corners, or |e1 x e2| not
   * above 1e-14 extent^2) is dropped.  A mesh given as points only has mesh_trinum 0; models assembled from tables have none. */
  int nmeshtri;
  int *mesh_triadr, *mesh_trinum;   /* [nmesh] */
  double* mesh_tri;                 /* [9*nmeshtri]: a, b, c per triangle, in the frame of mesh_vert */
  /* ---- appended for colour images (older fields keep their offsets) ----
   * <geom rgba> (its own, its default class's, or its <material>'s): mjh_render shades with r, g, b; the alpha is carried and not
   * used.  0.5 0.5 0.5 1 unless set [UPSTREAM, unverified here: MuJoCo's geom default].  NULL in a model assembled from tables: every
   * geom has the default. */
  double* geom_rgba;                /* [4*ngeom] */
  /* ---- appended for lights (older fields keep their offsets) ----
   * <light mode="fixed">: a frame attached to a body.  mjh_render's colour image takes the active lights when the engine's lighting
   * mode is 1 (mjh_render_set_lighting below, where the formula stands).  At most MJH_MAXLIGHT lights; a model assembled from tables
   * has none.  specular and attenuation are not modelled. */
  int nlight;
  int* light_bodyid;                      /* [nlight] */
  double *light_pos, *light_dir;          /* [3 nlight] each: position and unit direction in the body's frame */
  int *light_directional, *light_castshadow, *light_active;   /* [nlight] each, 0 / 1 */
  double *light_diffuse, *light_ambient;  /* [3 nlight] each: r, g, b, finite and not negative */
  double *light_cutoff, *light_exponent;  /* [nlight] each: spot cone half-angle in degrees, (0, 180]; spot exponent >= 0 */
  char** light_names;
  /* ---- appended for textures (older fields keep their offsets) ----
   * <texture type="2d">: texel tables, and per geom the texture its material names (materials stay flattened into the geom, as
   * geom_rgba is).  mjh_render's colour image samples them when the engine's texturing mode is 1 (mjh_render_set_texturing below,
   * where the mapping stands).  A model assembled from tables has ntex = 0 and NULL pointers. */
  int ntex, ntexdata;                     /* ntexdata in texels */
  int *tex_width, *tex_height, *tex_adr;  /* [ntex] each; tex_adr in texels */
  unsigned char* tex_rgb;                 /* [3*ntexdata]: row-major, row 0 first, R G B per texel */
  char** tex_names;
  int* geom_texid;                        /* [ngeom], -1 for none */
  double* geom_texrepeat;                 /* [2*ngeom] */
  int* geom_texuniform;                   /* [ngeom], 0 / 1 */
} mjh_model;

#define MJH_MAXLIGHT 8   /* lights a model can hold (they travel to the light kernel in its arguments) */
#define MJH_MAXTEXSIZE 4096        /* width and height of a texture: 1 ... MJH_MAXTEXSIZE each */
#define MJH_MAXTEXDATA (1 << 24)   /* the texels of all textures of a model total at most this */

/* ------------------------------------------------- model builder (host) */
/* Replaces the model-ingest boundary mj_loadXML (include/mujoco_sim/mj_util.h:190)
 * for programmatic scenes; an MJCF-subset loader is SURVEY.md §8-f F1. */
typedef struct mjh_builder mjh_builder;

mjh_builder* mjh_builder_create(void);
void mjh_builder_destroy(mjh_builder*);
void mjh_builder_set_option(mjh_builder*, const mjh_option*);
void mjh_builder_get_option(const mjh_builder*, mjh_option*);
void mjh_builder_set_capacity(mjh_builder*, int maxcon, int maxefc);
/* <compiler boundmass boundinertia>: lower bounds on the mass / principal inertias of every body except the world */
void mjh_builder_set_bounds(mjh_builder*, double boundmass, double boundinertia);
void mjh_builder_set_balanceinertia(mjh_builder*, int on);   /* <compiler balanceinertia> (mujoco_compile.cpp:157-160) */
/* returns body id (>0) ; parent 0 = world.  mass<=0 -> inertia inferred from geoms (density 1000) */
int mjh_builder_add_body(mjh_builder*, const char* name, int parent, const double pos[3],
                         const double quat[4], double gravcomp);
int mjh_builder_set_inertial(mjh_builder*, int body, double mass, const double ipos[3],
                             const double iquat[4], const double diaginertia[3]);
/* range==NULL -> unlimited.  Sentinels of add_geom / add_mesh_geom: friction NULL, condim / contype / conaffinity < 0 and
 * density < 0 mean "MuJoCo's default" (1 0.005 0.0001, 3, 1, 1, 1000); an explicit density 0 is a massless geom */
int mjh_builder_add_joint(mjh_builder*, const char* name, int body, int type, const double pos[3],
                          const double axis[3], const double range[2], double damping,
                          double stiffness, double armature, double frictionloss, double ref);
int mjh_builder_add_geom(mjh_builder*, const char* name, int body, int type, const double size[3],
                         const double pos[3], const double quat[4], const double friction[3],
                         int condim, int contype, int conaffinity, double density);
/* convex mesh asset (the <asset><mesh> of the reference's robots, pr2.xml:5-22): a vertex cloud, optionally with
 * triangles (volume, centre of mass and principal axes from the faces as mj_loadXML derives them; from the
 * bounding box otherwise).  Collides as its convex hull, like MuJoCo: the builder keeps the vertices that are
 * extreme along a dense set of directions.  scale may be NULL.  Returns the mesh id (>= 0) or a negative code. */
int mjh_builder_add_mesh(mjh_builder*, const double* vert, int nvert, const int* face, int nface, const double scale[3]);
int mjh_builder_add_mesh_stl(mjh_builder*, const char* path, const double scale[3]);   /* binary or ASCII STL, Wavefront OBJ (by extension) */
/* mesh geom: pos/quat place the MESH FILE's frame in the body, as <geom type="mesh" pos quat> does */
int mjh_builder_add_mesh_geom(mjh_builder*, const char* name, int body, int mesh, const double pos[3], const double quat[4],
                              const double friction[3], int condim, int contype, int conaffinity, double density);
/* height field asset (<asset><hfield nrow ncol size elevation>): elevation row-major [nrow*ncol] (NULL: zeros), normalised to
 * [0, 1] at compile time (minus the minimum, divided by max - min when that is non-zero); size = radius_x, radius_y,
 * elevation_z, base_z, each > 0; nrow, ncol >= 2.  Returns the hfield id (>= 0) or a negative code. */
int mjh_builder_add_hfield(mjh_builder*, const char* name, int nrow, int ncol, const double size[4], const double* elevation);
/* hfield geom: on a static body only (body_weldid 0; otherwise MJH_ERR_UNSUPPORTED), massless.  It collides with spheres,
 * capsules, ellipsoids, cylinders, boxes and meshes as triangular prisms, one contact per prism, at most 50 per pair.
 * (mjh_builder_add_geom with type MJH_GEOM_HFIELD keeps a geom without an asset: it has no pairs.) */
int mjh_builder_add_hfield_geom(mjh_builder*, const char* name, int body, int hfield, const double pos[3], const double quat[4],
                                const double friction[3], int condim, int contype, int conaffinity);
int mjh_builder_add_exclude(mjh_builder*, int body1, int body2);
int mjh_builder_add_eq_joint(mjh_builder*, int joint1, int joint2, const double polycoef[5]);
/* <equality><connect body1 body2 anchor> / <weld body1 body2 anchor torquescale> (body2 = 0: the world).  connect: `anchor`
 * in body1's frame; weld: in body2's frame (NULL = its origin), the relative pose is the one at qpos0.  MjSim::init_references
 * emits <weld body1="X" body2="X_ref" torquescale="0.9"/> against a mocap clone of X (mj_sim.cpp:933-938). */
int mjh_builder_add_eq_connect(mjh_builder*, int body1, int body2, const double anchor[3]);
int mjh_builder_add_eq_weld(mjh_builder*, int body1, int body2, const double anchor[3], double torquescale);
/* <body mocap="true">: a child of the world without joints whose pose is set per environment at run time */
int mjh_builder_set_mocap(mjh_builder*, int body);
/* <site> and <sensor><force site=.../><torque site=.../> */
int mjh_builder_add_site(mjh_builder*, const char* name, int body, const double pos[3], const double quat[4]);
int mjh_builder_add_sensor(mjh_builder*, const char* name, int type /* mjh_sensor */, int site);
/* <camera> (fixed mode): returns the camera id.  pos / quat NULL: the identity (quat is normalised); fovy <= 0: MuJoCo's default of 45
 * degrees; fovy >= 180 or a bad body: MJH_ERR_ARG */
int mjh_builder_add_camera(mjh_builder*, const char* name, int body, const double pos[3], const double quat[4], double fovy);
/* <geom rgba>: the colour of geom `geom` (the id an mjh_builder_add_*geom call returned; the compiled model may number it differently,
 * the colour follows it).  A bad id, a NULL pointer or a component outside [0, 1]: MJH_ERR_ARG, nothing is changed. */
int mjh_builder_set_geom_rgba(mjh_builder*, int geom, const double rgba[4]);
/* <light> (fixed mode): returns the light id.  pos / dir in the body's frame; dir is normalised.  NULL pointers take the defaults
 * [UPSTREAM, unverified here: MuJoCo's light defaults]: pos 0 0 0, dir 0 0 -1, diffuse 0.7 0.7 0.7, ambient 0 0 0; the XML defaults of
 * the scalars are positional, castshadow on (directional / castshadow < 0 take them), cutoff 45 degrees and exponent 10 (given
 * explicitly: the loader passes them).  The light is active.  A bad body, a zero
 * or non-finite dir, a negative or non-finite colour component, cutoff outside (0, 180], a negative or non-finite exponent, or a light
 * beyond MJH_MAXLIGHT: MJH_ERR_ARG, nothing is added.  Like a camera the light follows its body through the compile step's reordering. */
int mjh_builder_add_light(mjh_builder*, const char* name, int body, const double pos[3], const double dir[3], int directional,
                          int castshadow, const double diffuse[3], const double ambient[3], double cutoff_deg, double exponent);
int mjh_builder_set_light_active(mjh_builder*, int light, int on);   /* <light active>: the model's light_active (a bad id: MJH_ERR_ARG) */
/* <texture type="2d">.  Limits: width and height 1 ... MJH_MAXTEXSIZE each, the texels of all textures of a model at most
 * MJH_MAXTEXDATA.  Beyond them, or with a NULL pointer / a bad enum / a colour component outside [0, 1]: MJH_ERR_ARG, nothing is added.
 * mjh_builder_add_texture takes the caller's texels (3 width height bytes, row-major, row 0 first, R G B) and returns the texture id.
 * mjh_builder_add_texture_builtin generates them on the host; MuJoCo is on no machine this runs on, so the definitions are these
 * [UPSTREAM, unverified here: MuJoCo's builtin textures and marks]:
 *   a byte is (int)(255 c + 0.5) for c in [0, 1];
 *   flat: every texel is rgb1;
 *   checker: texel (row j, column i) is rgb1 where (j < H/2) == (i < W/2) (integer division), rgb2 elsewhere: one repetition of the
 *     texture is 2 x 2 squares;
 *   gradient: x = 2i/(W-1) - 1, y = 2j/(H-1) - 1 (0 where the dimension is 1), r = min(1, sqrt(x^2 + y^2)), colour rgb1 (1 - r) + rgb2 r;
 *   mark edge: row 0, row H-1, column 0 and column W-1 take markrgb; mark cross: row H/2 and column W/2 take markrgb.
 * NULL rgb1 / rgb2 / markrgb take 0.8 0.8 0.8 / 0.5 0.5 0.5 / 0 0 0 [UPSTREAM, unverified here: MuJoCo's texture defaults]. */
enum mjh_texbuiltin { MJH_TEXBUILTIN_FLAT = 0, MJH_TEXBUILTIN_CHECKER = 1, MJH_TEXBUILTIN_GRADIENT = 2 };
enum mjh_texmark { MJH_TEXMARK_NONE = 0, MJH_TEXMARK_EDGE = 1, MJH_TEXMARK_CROSS = 2 };
int mjh_builder_add_texture(mjh_builder*, const char* name, int width, int height, const unsigned char* rgb);
int mjh_builder_add_texture_builtin(mjh_builder*, const char* name, int builtin, int mark, int width, int height,
                                    const double rgb1[3], const double rgb2[3], const double markrgb[3]);
/* a material's texture, texrepeat, texuniform on geom `geom` (a builder geom id, as for mjh_builder_set_geom_rgba).  tex = -1 clears
 * (texrepeat may then be NULL).  NULL texrepeat is 1 1; its components must be finite and > 0.  A bad geom or texture id, a bad
 * texrepeat: MJH_ERR_ARG, nothing is changed.  A mesh geom takes no texture (its texture coordinates are not kept): MJH_ERR_ARG. */
int mjh_builder_set_geom_texture(mjh_builder*, int geom, int tex, const double texrepeat[2], int texuniform);
/* compile: derives inertias, qpos0, invweight0, meaninertia, rbound, pair list */
mjh_model* mjh_builder_compile(mjh_builder*);
void mjh_model_destroy(mjh_model*);
/* (the mesh assets — mesh_vert and the hull planes — are shared by the copies of mjh_model_replicate) */
/* Sub-wave packing for small models (nv of a few, a handful of bodies: the C1 / C3 / C5 scenes): `copies` independent
 * instances of every moving body tree in ONE model, sharing the static geometry (world / welded-to-world geoms) and
 * never colliding with each other.  An engine created from the result steps `copies` environments per wavefront:
 * row w of every state array holds the qpos / qvel / ... of environments w*copies .. w*copies+copies-1 back to back
 * (copy c at offset c*nq, c*nv).  What the instances of one wavefront share: the solver's termination test (sweeps
 * continue until the slowest instance has converged), `time`, the statistics row and the bad-state reset.  Contact
 * and row capacities scale with `copies`.  Returns a new model (mjh_model_destroy) or NULL. */
mjh_model* mjh_model_replicate(const mjh_model* m, int copies);
int mjh_name2id(const mjh_model*, int objtype /*0 body,1 joint,2 geom,3 site,4 sensor,5 camera,6 light,7 texture*/, const char* name);
const char* mjh_id2name(const mjh_model*, int objtype, int id);

/* MJCF-subset loader: replaces load_XML -> mj_loadXML (include/mujoco_sim/mj_util.h:185-193) for the element
 * subset the reference models use on the step path (see csrc/mjcf_loader.cpp).  Returns NULL + mjh_last_error()
 * on failure; mjh_load_note() lists what was skipped (mesh geoms, <include>, default classes, ...). */
mjh_model* mjh_load_mjcf_string(const char* xml);
mjh_model* mjh_load_mjcf_file(const char* path);
/* one model from several files: the reference composes a world file and robot files into one MJCF before mj_loadXML
 * (MjSim::init, mj_sim.cpp:573-710).  <option> comes from the first file; names must be unique across files. */
mjh_model* mjh_load_mjcf_files(const char* const* paths, int n);
const char* mjh_load_note(void);
/* The loader options of ONE call (what MjSim::init_tmp reads from rosparams and writes into the files before mj_loadXML): the
 * mjh_load_set_* functions below keep per-THREAD settings for all later loads; this variant takes them as an argument and
 * leaves the thread's settings untouched. */
typedef struct mjh_load_options {
  double boundmass, boundinertia;   /* floor for <compiler boundmass boundinertia>: the reference writes 1e-6 / 1e-6 (mj_sim.cpp:584-590) */
  int robot_gravcomp;               /* ~disable_gravity: -1 keep the files' values, 0 / 1 written on every robot body (mj_sim.cpp:301-310) */
  int load_meshes;                  /* 1: mesh assets are read and collide as hulls; 0: mesh geoms are dropped (and noted) */
  unsigned odom_joints;             /* ~add_odom_joints mask: bits 0..5 = lin x y z, ang x y z (mj_sim.cpp:337-415) */
  int nrobot_pose;                  /* ~pose_init entries (mj_sim.cpp:312-335): root body names and x y z roll pitch yaw each */
  const char* const* robot_pose_body; const double* robot_pose;
  int parent_child_exclude;         /* disable_parent_child_collision_level (mujoco_sim.launch:7; mujoco_compile.cpp:250-290): see mjh_load_set_parent_child_exclude; 0 adds nothing */
} mjh_load_options;
void mjh_load_default_options(mjh_load_options*);
mjh_model* mjh_load_mjcf_files_opt(const char* const* paths, int n, const mjh_load_options* options);
/* 1 (default): <asset><mesh> files are read and mesh geoms collide as convex hulls; 0: mesh geoms are dropped (and
 * listed in mjh_load_note), which leaves the primitive collision geometry only */
void mjh_load_set_mesh_mode(int mode);
/* 0 (default): <texture> is not read and a material's texture / texrepeat / texuniform get the "ignored material attribute" note
 * (the compiled model has ntex = 0).  1: <asset><texture type="2d" builtin="flat|checker|gradient"> becomes a texture of the model
 * (mjh_builder_add_texture_builtin) and a material's texture, texrepeat (1 1) and texuniform (false) go to every geom that names the
 * material, whichever colour the geom takes.  Skipped with a note, the geoms keeping their plain colour: cube and skybox textures,
 * file textures (no image decoder), mark="random", a texture over the limits, a material that names an unknown texture, a texture
 * on a mesh geom.  Thread-local, like the other load settings. */
void mjh_load_set_textures(int mode);
/* rosparam ~disable_gravity of the reference (robot.yaml:19, default true): MjSim::init_tmp rewrites gravcomp on EVERY
 * body of a robot file — 1 if set, 0 otherwise (mj_sim.cpp:301-310).  mode 1 / 0 does the same to the bodies of the files
 * after the first one in mjh_load_mjcf_files; -1 (default) keeps what the files say. */
void mjh_load_set_robot_gravcomp(int mode);
/* rosparam ~add_odom_joints (robot.yaml; mj_sim.cpp:337-415): the root body of every robot file gets the joints
 * "<root>_lin_odom_{x,y,z}_joint" (slide) / "<root>_ang_odom_{x,y,z}_joint" (hinge) selected by mask bits 0..5
 * (lin x y z, ang x y z), with the reference's rule that a planar linear axis comes along when the other one and the yaw
 * (or, for z, the pitch) are selected.  Resolve their dofs with mjh_name2id and pass them to mjh_set_odom_dofs. */
void mjh_load_set_odom_joints(unsigned mask);
/* launch argument disable_parent_child_collision_level of the reference (mujoco_sim.launch:7, default 1): its mujoco_compile writes
 * <exclude> pairs between every body and its first `level` ancestors into the compiled robot file (mujoco_compile.cpp:250-290).
 * Per-thread setting for all later loads; 0 (default) adds nothing (adjacent bodies are filtered by the model compiler anyway,
 * as MuJoCo's filterparent does).  Applied to robot files only — the files after the first of mjh_load_mjcf_files, or the one file of a
 * single-file load —, to the bodies that file adds; the walk ends at the file's top level (the reference names the robot's geom-less
 * wrapper body there, mujoco_compile.cpp:272-276: no collision is excluded by that pair). */
void mjh_load_set_parent_child_exclude(int level);
/* rosparam ~pose_init (mj_sim.cpp:312-335): position and roll / pitch / yaw (radians, tf2 setRPY) written onto the root body
 * of a robot file, by body name; pose NULL removes the entry, root_body NULL removes all */
void mjh_load_set_robot_pose(const char* root_body, const double pose[6]);
/* per-thread floor for <compiler boundmass boundinertia> of every file loaded afterwards: the reference writes
 * 1e-6 / 1e-6 into each file before mj_loadXML (mj_sim.cpp:584-590) */
void mjh_load_set_bounds(double boundmass, double boundinertia);

/* ------------------------------------------------------ scene builders */
/* SURVEY.md §8-d configs, as programmatic models.  `seed_base+env` seeds PCG32. */
mjh_model* mjh_scene_s24(void); /* 4 free boxes in a walled pen on the empty.xml floor  */
mjh_model* mjh_scene_s24_pen(double pen_half, int maxcon); /* the same scene with another pen (S24 itself: 0.175, 40); bench.py `s24d`: a narrow pen, ~30 contacts */
/* per-env S24 randomisation: fills qpos0[nenv*nq] and the per-env parameter tables
 * (each out pointer may be NULL).  Box half-extents U[0.05,0.125]^3.             */
int mjh_scene_s24_randomize(const mjh_model*, int env0, int nenv, unsigned seed_base,
                            double* qpos, double* geom_size, double* geom_rbound,
                            double* body_mass, double* body_inertia,
                            double* body_invweight0, double* dof_invweight0);
/* per-env randomisation of any scene of free boxes (C2): half-extents U[0.05,0.125]^3 with the mass /
 * inertia / inverse weights that follow, lattice position = the model's qpos0 + U[-jitter,jitter]^3, uniformly random
 * orientation; same table layout and seeding as mjh_scene_s24_randomize */
int mjh_scene_boxes_randomize(const mjh_model*, int env0, int nenv, unsigned seed_base, double jitter,
                              double* qpos, double* geom_size, double* geom_rbound,
                              double* body_mass, double* body_inertia,
                              double* body_invweight0, double* dof_invweight0);
mjh_model* mjh_scene_pendulum(void);          /* model/test/pendulum.xml restated (C1/C5) */
mjh_model* mjh_scene_arm7(int gravcomp);      /* 7-hinge Panda-like chain with limits (C3) */
mjh_model* mjh_scene_boxpile(int nbox);       /* nbox free boxes over the floor (C2 family) */

/* --------------------------------------------------------------- engine */
typedef struct mjh_engine mjh_engine;

/* Create an engine for `nenv` environments on HIP device `device`.
 * Replaces mj_makeData (mj_sim.cpp:816,835; mj_ros.cpp:571) + init_malloc
 * (mj_sim.cpp:563-571: ddq/dq/tau buffers).  `stream` is a hipStream_t (may be
 * NULL for the default stream); all kernels are launched on it. */
int mjh_create(const mjh_model* model, int nenv, int device, void* stream, mjh_engine** out);
void mjh_destroy(mjh_engine*); /* mj_deleteData/mj_deleteModel, mj_main.cpp:232-233 */

/* mj_step1 (mj_main.cpp:83): position + velocity stages, then the control
 * callback MjSim::controller (mj_sim.cpp:1055-1077) as a built-in device stage.
 * The launch itself is deferred to the next entry point: the reference calls
 * MjHWInterface::read() = mj_inverse right behind mj_step1 (mj_main.cpp:83-94), and
 * mjh_step1 + mjh_inverse then go out as ONE launch sharing the position and velocity
 * stages (the literal loop: 5.3 -> 5.9 M env-steps/s on S24); any other entry point
 * first issues the plain step1 launch, so the order of effects is the order of the
 * calls.  MJH_LAZY_STEP1=0 launches immediately. */
int mjh_step1(mjh_engine*);
/* mj_step2 (mj_main.cpp:108) then MjSim::set_odom_vels (mj_main.cpp:110). */
int mjh_step2(mjh_engine*);
/* n fused steps: step1 -> [inverse if with_inverse] -> step2, one launch per step
 * window; with_inverse reproduces the per-step mj_inverse of MjHWInterface::read
 * (mj_hw_interface.cpp:61). */
int mjh_step(mjh_engine*, int nsteps, int with_inverse);
/* mj_inverse (mj_hw_interface.cpp:61): fills qfrc_inverse. */
int mjh_inverse(mjh_engine*);
/* mj_forward (mj_ros.cpp:608,1421). */
int mjh_forward(mjh_engine*);
/* mj_mulM (mj_sim.cpp:1057): res = M(q)*vec for envs [env0, env0+n); host doubles [n*nv]. */
int mjh_mulM(mjh_engine*, int env0, int n, const double* vec, double* res);
int mjh_synchronize(mjh_engine*);

/* MjHWInterface::write (mj_hw_interface.cpp:73-91): ddq = effort command
 * (interpreted as desired acceleration), dq = velocity command; [n*nv] each,
 * either may be NULL.  Consumed (and zeroed, mj_sim.cpp:1075-1076) by the next step1.
 * The buffers are read before the call returns; a call of at most 4096 values goes through a
 * host-mapped staging ring and does not wait for the device (stream-ordered in front of the
 * range's next step launch), larger ones copy and wait. */
int mjh_set_cmd(mjh_engine*, int env0, int n, const double* ddq, const double* dq);
/* Device forms of the control side of the loop (mjh_set_cmd_device, mjh_set_pd_target_device, mjh_set_xfrc_applied_device,
 * mjh_get_joint_state_device, mjh_reset_device): a controller or policy on the same GPU exchanges actions, joint state and episode resets
 * with the engine without a host copy, a conversion or a synchronisation.
 * Contract of all five: device buffers are dense fp32 rows [n][width]; row i belongs to env env0 + i.  A call is enqueued and returns
 * without waiting for the device; it reads or writes its buffers in stream order on the engine's stream (the stream given to mjh_create).
 * The caller orders the producer (setters, reset) or the consumer (getter) of a buffer on that stream and keeps the buffer alive until the
 * stream has passed the call.  Bits are copied: for fp32-representable values a setter leaves exactly what its host counterpart leaves
 * (which rounds double to float).  The pointers are not inspected: a host address handed in here faults on the device.
 * Not forwarded by mjh_group; not meant to be captured into a caller's graph.
 * mjh_set_cmd_device: [n][nv] each, either may be NULL (both: no-op).  Like mjh_set_cmd it keeps a hand-over pending between mjh_step1 and
 * mjh_step2, and a range inside one cohort touches that cohort's stream only. */
int mjh_set_cmd_device(mjh_engine*, int env0, int n, const float* d_ddq, const float* d_dq);
/* In-engine joint-space PD effort controller for ALL environments.  The reference closes this loop on the host for its one
 * environment: read() -> controller_manager->update() -> write() (mj_main.cpp:86-106) with ros_control effort controllers
 * (PID p 200 d 50: model/ontology/box/box.yaml:5-13) whose output MjSim::controller treats as a desired acceleration
 * (mj_sim.cpp:1057).  With thousands of environments the same law runs on the device in front of every step:
 * ddq[d] = kp (target[d] - qpos[d]) - kd qvel[d] on every hinge / slide dof (other dofs untouched), consumed by the controller
 * stage of mj_step1 exactly like a command written with mjh_set_cmd.  kp = kd = 0 switches it off.  Targets default to qpos0;
 * mjh_set_pd_target takes [n*nv] values indexed by dof. */
int mjh_set_pd_controller(mjh_engine*, double kp, double kd);
int mjh_set_pd_target(mjh_engine*, int env0, int n, const double* target);
/* device form (contract: see mjh_set_cmd_device): d_target [n][nv]; MJH_ERR_STATE until the controller has been enabled */
int mjh_set_pd_target_device(mjh_engine*, int env0, int n, const float* d_target);
/* which dofs are "controlled" (MjSim::controlled_joints, mj_sim.cpp:1058-1063): mask[nv] */
int mjh_set_controlled_dofs(mjh_engine*, const int* mask);
/* MjSim::set_odom_vels (mj_sim.cpp:1079-1153): dof ids of the 6 odom joints of one
 * robot (-1 = absent) and the commanded twist per env [n*6] */
int mjh_set_odom_dofs(mjh_engine*, const int lin_dof[3], const int ang_dof[3],
                      const int ang_qpos[3]);
int mjh_set_odom_vel(mjh_engine*, int env0, int n, const double* twist);

/* MjHWInterface::read (mj_hw_interface.cpp:62-70): waits for the steps queued on the range's
 * stream (one cohort's, if the range lies inside a cohort); up to 16384 values are packed by one
 * small kernel into host-mapped memory (one synchronisation), larger ranges take strided copies */
int mjh_get_joint_state(mjh_engine*, int env0, int n, double* qpos, double* qvel,
                        double* qfrc_inverse);
/* device form (contract: see mjh_set_cmd_device): d_qpos [n][nq], d_qvel [n][nv], d_qfrc_inverse [n][nv], any may be NULL; the rows are
 * written behind the steps queued on the range's stream, nothing is waited for (qfrc_inverse is what the caller's mjh_inverse left) */
int mjh_get_joint_state_device(mjh_engine*, int env0, int n, float* d_qpos, float* d_qvel, float* d_qfrc_inverse);
/* d->xpos / d->xquat readers (mj_ros.cpp:2100-2147) */
int mjh_get_body_state(mjh_engine*, int env0, int n, double* xpos, double* xquat);
/* d->geom_xpos / geom_xmat readers (mj_ros.cpp:1968-2094) */
int mjh_get_geom_state(mjh_engine*, int env0, int n, double* geom_xpos, double* geom_xmat);
/* full state: time, qpos, qvel, qacc_warmstart (add_old_state, mj_sim.cpp:465-558).  `time` is kept in fp64 on the device
 * (d->time is mjtNum: the ROS stamps, the 10 kHz controller gate and the real-time factor of mj_main.cpp:85,115-163 read
 * it): after n steps it equals n * opt.timestep to fp64 round-off, however long the simulation runs; only the packed
 * fp32 publish slice (mjh_export_state_device) rounds it */
int mjh_get_state(mjh_engine*, int env0, int n, double* time, double* qpos, double* qvel,
                  double* qacc_warmstart);
int mjh_set_state(mjh_engine*, int env0, int n, const double* time, const double* qpos,
                  const double* qvel, const double* qacc_warmstart);
/* (qacc and qacc_warmstart are one array on the device: after every solve qacc_warmstart = qacc, as mj_advance leaves them;
 * writing a warm start through mjh_set_state therefore also sets the qacc a following mjh_inverse reads)
 * other per-env vectors by name: "qacc","qfrc_bias","qfrc_applied","qfrc_passive",
 * "qfrc_constraint","qfrc_inverse","qacc_smooth","energy"(2) */
int mjh_get_field(mjh_engine*, const char* name, int env0, int n, double* out);
/* per-env solver statistics: ncon, nefc, solver iterations, flags (bit0 contact overflow,
 * bit1 row overflow, bit2 NaN reset) — int[n*4] */
int mjh_get_stats(mjh_engine*, int env0, int n, int* out);
/* contacts of ONE env (debug/parity): dist[maxcon], pos[3*maxcon], frame[9*maxcon], geom[2*maxcon]; returns ncon or <0.
 * Read-only: runs the position stage of that env into a scratch buffer; state, statistics, warm start and time are untouched
 * (it may be called between mjh_step1 and mjh_step2) */
int mjh_get_contacts(mjh_engine*, int env, double* dist, double* pos, double* frame, int* geom);

/* d->xfrc_applied (mj_sim.cpp:499 carries it across a model change): Cartesian force (3) and torque (3) per body, world
 * frame, applied at the body's centre of mass; [n * 6*nbody].  Enters qfrc_smooth of every step until changed. */
int mjh_set_xfrc_applied(mjh_engine*, int env0, int n, const double* xfrc);
/* device form (contract: see mjh_set_cmd_device): d_xfrc [n][6*nbody].  The first call of either form on an engine allocates the array
 * and waits for the device once; none after it does. */
int mjh_set_xfrc_applied_device(mjh_engine*, int env0, int n, const float* d_xfrc);
int mjh_get_xfrc_applied(mjh_engine*, int env0, int n, double* xfrc);
/* d->sensordata (mj_ros.cpp:1933-1966 reads sensordata[sensor_adr[i] .. +3] of every force / torque sensor): [n * nsensordata],
 * computed at the end of mj_step2's forward part (mj_sensorAcc), i.e. the values of the LAST step */
int mjh_get_sensordata(mjh_engine*, int env0, int n, double* sensordata);
/* pose of mocap body `mocapid` in envs [env0, env0+n): pos[n*3], quat[n*4] (either may be NULL) — d->mocap_pos / mocap_quat,
 * what the reference's `~receive` mode drives (mj_sim.cpp:847-960) */
int mjh_set_mocap_pose(mjh_engine*, int env0, int n, int mocapid, const double* pos, const double* quat);
/* per-env model parameters (enum mjh_env_param) */
int mjh_set_env_param(mjh_engine*, int which, int env0, int n, const double* values);
/* MjRos::reset_robot (mj_ros.cpp:569-609): back to qpos0 (or the per-env initial
 * qpos set by mjh_set_initial_qpos), zero qvel/qacc/warmstart/time */
/* State transplant after a model change (reference: add_old_state(), mj_sim.cpp:465-558, run when spawn/destroy or a
 * robot reload recompiles the model): for every body of `from` whose NAME also exists in `to`, copy its joints' state
 * of envs [0, min(nenv)) — time, qvel, qacc_warmstart, qfrc_applied and qacc per dof if the dof counts match, qpos if the
 * joint counts match.  qpos_mode 0 is literal: the reference copies body_jntnum scalars of qpos (one per joint, so a free
 * body keeps only its x and otherwise takes the pose baked into the new model, mj_sim.cpp:613-623); qpos_mode 1 copies
 * every qpos scalar of the body's joints.  Returns the number of bodies matched, or a negative code. */
int mjh_transplant_state(mjh_engine* from, mjh_engine* to, int qpos_mode);
int mjh_set_initial_qpos(mjh_engine*, int env0, int n, const double* qpos);
int mjh_reset(mjh_engine*, const int* env_ids, int n);
/* (env_ids NULL: every env, and the launch scheduling starts over; a list of n >= 2 ids, in any order, duplicates allowed, is one upload
 * and one launch, and leaves the scheduling state alone like a single id)
 * Masked reset from device buffers (contract: see mjh_set_cmd_device): every env of [env0, env0 + n) with d_mask[i] != 0 (d_mask NULL:
 * all of them) gets what mjh_reset does to one env: qpos = its initial qpos, qvel / qacc_warmstart / the pending command / time / solver
 * statistics = 0, its contact report cleared.  With d_qpos [n][nq] or d_qvel [n][nv] a selected env takes its row from there instead, as
 * given (not normalised, like mjh_set_state); rows of envs that are not selected are not read, and those envs are not written.  Drops a
 * hand-over pending between mjh_step1 and mjh_step2. */
int mjh_reset_device(mjh_engine*, int env0, int n, const unsigned char* d_mask, const float* d_qpos, const float* d_qvel);

/* spawn / destroy as per-env slot toggling (reference: spawn_objects / destroy_objects services,
 * mj_ros.cpp:859-1507, which re-compile the whole model): an inactive slot does not collide and is frozen.
 * Toggleable are the last 32 bodies of the model (all of them, except the world, in a model of up to 32 bodies):
 * declare the object pool after the robot. */
int mjh_set_slot_active(mjh_engine*, int env0, int n, int body, int active);
/* the services take LISTS (mujoco_msgs SpawnObject.objects[] / DestroyObject.names[], mj_ros.cpp:859-904,1430-1507): one call,
 * one upload and one small kernel for n (env, body) pairs — activate + pose (pos[n*3], quat[n*4] or NULL) + twist (vel[n*6] or
 * NULL: linear world, angular body frame, as qvel of a free joint) / deactivate */
int mjh_spawn_objects(mjh_engine*, int n, const int* env, const int* body, const double* pos, const double* quat, const double* vel);
int mjh_destroy_objects(mjh_engine*, int n, const int* env, const int* body);
/* initial pose / twist of a spawned free body (mj_ros.cpp:1406-1412) */
int mjh_set_body_pose(mjh_engine*, int env, int body, const double pos[3], const double quat[4], const double vel[6]);

/* Batched ray casting: mj_ray for every environment (the reference's robots carry laser scanners: the hsrb4s base scanner, PR2's
 * tilt laser mount; MuJoCo answers such queries with mj_ray and the rangefinder sensor).  nray rays against the geoms of envs
 * [env0, env0+n) at the envs' present qpos.  dist is the smallest x >= 0 for which pnt + x vec lies on the surface of a visible
 * geom — in units of |vec|, vec is not normalised for the caller —, geomid that geom; a miss is dist = -1, geomid = -1.
 *   plane: front (+z) face only, bounded by size[0] / size[1] where those are > 0;
 *   sphere, capsule, ellipsoid, cylinder (flat caps), box: nearest non-negative root (an origin inside hits the far surface);
 *   height field: the solid the collision code uses (two triangles per cell sharing the diagonal (r,c)-(r+1,c+1), side walls and
 *     base down to -size[3]), hit at its nearest surface from any side;
 *   mesh geoms: invisible by default (mode 0); with mjh_ray_set_mesh_mode(engine, 1) a mesh geom is hit at the nearest non-negative x
 *     on its convex hull (mesh_plane: the hull of the kept vertices, the solid the narrow phase collides), and an origin inside hits
 *     the far surface, like the other bounded types.  mj_ray itself intersects the mesh file's triangles: for a convex mesh the two
 *     agree, for a non-convex one the ray sees the collision hull unless mjh_ray_set_mesh_surface (below) selects the triangles.
 *     bodyexclude, flg_static, inactive slots and cutoff apply to mesh geoms like any other.  A mesh geom's hull is that of the
 *     model's mesh_vert: per-env geom sizes do not rescale it, as they do not in the narrow phase.
 *   hfield geoms without an asset are invisible; mjh_ray_skipped_geoms counts what mode 0 cannot see.
 * A geom of a body whose spawn / destroy slot is inactive in an env is invisible there; geom sizes are the env's own where per-env
 * sizes are set (mjh_set_env_param).  Call-sequence rules are those of mjh_get_geom_state (a pending mjh_step1 is issued first and a
 * window hand-over is dropped); nothing of the envs' state, statistics or time is written. */
typedef struct mjh_ray_options {
  int site;         /* >= 0: pnt / vec are given in this site's frame and follow it per env; -1: world frame */
  int bodyexclude;  /* geoms of this body are invisible (mj_ray's bodyexclude); -1: none */
  int flg_static;   /* 0: geoms of static bodies (body_weldid 0) are invisible; 1: visible */
  int per_env;      /* 0: one ray set [nray] shared by all envs; 1: pnt / vec are [n][nray] */
  double cutoff;    /* > 0: hits with dist beyond it are misses (rangefinder cutoff); <= 0: none */
} mjh_ray_options;
void mjh_ray_default_options(mjh_ray_options*);   /* -1, -1, 1, 0, 0 */
/* host pointers, doubles: converts, calls the device form and synchronises.  options may be NULL (the defaults).  A zero vec, nray <= 0,
 * an env range, site or body id out of range return MJH_ERR_ARG and launch nothing. */
int mjh_ray(mjh_engine*, int env0, int n, int nray, const double* pnt, const double* vec,
            const mjh_ray_options*, double* dist /*[n][nray]*/, int* geomid /*[n][nray]*/);
/* device pointers, fp32: enqueued on the engine's stream, returns without synchronising; the results are valid after
 * mjh_synchronize (a zero vec cannot be refused here: such a ray misses) */
int mjh_ray_device(mjh_engine*, int env0, int n, int nray, const float* d_pnt, const float* d_vec,
                   const mjh_ray_options*, float* d_dist, int* d_geomid);
int mjh_ray_skipped_geoms(const mjh_model*);     /* geoms no ray can see in mesh mode 0 (mesh geoms, hfield geoms without an asset) */
/* how the rays of this engine treat mesh geoms: 0 (default) invisible, 1 hit as the convex hull; any other mode returns MJH_ERR_ARG and
 * changes nothing.  Takes effect with the next ray call (the geom table of the mode is uploaded on that call's stream order). */
int mjh_ray_set_mesh_mode(mjh_engine*, int mode);
int mjh_ray_get_mesh_mode(const mjh_engine*);
/* What a VISIBLE mesh geom is to a ray (the mesh mode keeps its meaning and its two values: 0 mesh geoms are invisible, 1 visible).
 * MJH_RAY_SURFACE_HULL (default): the convex hull, as above.  MJH_RAY_SURFACE_TRIANGLES: a mesh geom whose asset has triangles
 * (mesh_trinum > 0) is hit on them, as mj_ray does: dist is the smallest x >= 0 with pnt + x vec on ANY triangle of the mesh, from
 * either side — so an origin inside a closed mesh hits the far surface, like the other bounded types, a hole the hull fills is open,
 * and a mesh without volume (a flat panel: triangles but no hull planes) becomes visible.  A mesh geom without triangles keeps its
 * hull, or stays invisible if it has no hull planes either.  In units of |vec|; bodyexclude, flg_static, cutoff, the slot masks and the
 * lower geom id on a tie are unchanged; per-env geom sizes do not rescale a mesh, as in hull mode.  A triangle includes its edges
 * with a few fp32 ulps of slack: a ray through a shared edge or vertex of a watertight mesh does not pass
 * between two triangles.  mjh_ray and mjh_depth both obey the switch; mjh_ray_skipped_geoms keeps its mode-0 meaning.  The triangle
 * tables (a bounding-volume hierarchy per mesh asset, built on the host) are uploaded by the first ray or depth call issued with the
 * triangles selected: an engine that never selects them pays nothing.  Any other value returns MJH_ERR_ARG and changes nothing.
 * [UPSTREAM, unverified here] MuJoCo 2.3.7's mj_rayMesh tests every face of the mesh, two-sided. */
enum { MJH_RAY_SURFACE_HULL = 0, MJH_RAY_SURFACE_TRIANGLES = 1 };
int mjh_ray_set_mesh_surface(mjh_engine*, int surface);
int mjh_ray_get_mesh_surface(const mjh_engine*);

/* Depth images: every env's view through a camera of the model, as tiled depth / segmentation images (the observation vision
 * policies train on).  The rays are generated on the device from the camera's intrinsics and its body's pose in each env: no ray
 * buffer is uploaded, and a camera on a moving body follows it per env.
 *   Pixel (i, j) is row i from the top, column j from the left; its ray starts at the camera origin and goes through the pixel's
 *   centre: in the camera frame d = (a t (2 (j + 1/2) / W - 1), t (1 - 2 (i + 1/2) / H), -1) with t = tan(fovy / 2), a = W / H.
 *   d.z = -1, so the ray parameter of the hit (in units of |d|) is the depth along the optical axis, what a depth buffer holds
 *   (range = 0); range = 1 multiplies it by |d|: the Euclidean distance from the camera origin.  A miss is depth -1, geomid -1.
 *   Everything else is mjh_ray's on the same engine: the semantics per geom type (a camera inside a geom sees its far surface),
 *   inactive slots, per-env geom sizes, mjh_ray_set_mesh_mode and mjh_ray_set_mesh_surface (they govern depth images too), the lower geom id on an exact fp32
 *   tie, and the call-sequence rules (a pending mjh_step1 goes out first, a window hand-over is dropped).  Nothing of state,
 *   statistics, warm start or time is written.
 *   cull: each 8 x 8 pixel tile walks only the bounded geoms whose bounding sphere touches the tile's cone; cull = 0 makes every
 *   tile visit every geom.  The two give the same bits (the cull may never cost a hit).
 * A model without cameras, a camera or body id out of range, a non-positive size (or n * width * height of 2^30 or more), an env range
 * out of bounds or a NULL depth pointer return MJH_ERR_ARG and launch nothing. */
typedef struct mjh_depth_options {
  int camera;          /* camera id */
  int width, height;   /* pixels, each >= 1; n * width * height below 2^30 */
  int bodyexclude;     /* geoms of this body are invisible; -1: none (MuJoCo renders the camera's own body: -1 is the default) */
  int flg_static;      /* as mjh_ray_options */
  int range;           /* 0: depth along the optical axis (what a depth buffer holds); 1: Euclidean distance from the camera origin */
  int cull;            /* 1 (default): tile culling on; 0: every tile visits every geom -- same results bit for bit (debug / test) */
  double cutoff;       /* > 0: a reported value beyond it is a miss (far plane); <= 0: none */
} mjh_depth_options;
void mjh_depth_default_options(mjh_depth_options*);   /* 0, 64, 64, -1, 1, 0, 1, 0 */
/* device pointers; enqueued on the engine's stream, no synchronisation; d_geomid may be NULL.  options may be NULL (the defaults) */
int mjh_depth_device(mjh_engine*, int env0, int n, const mjh_depth_options*, float* d_depth /*[n][height][width]*/, int* d_geomid);
/* host pointers (fp32 images; geomid may be NULL): calls the device form through an engine-owned staging buffer and synchronises */
int mjh_depth(mjh_engine*, int env0, int n, const mjh_depth_options*, float* depth, int* geomid);

/* Lidar range images: every env's scan from a site of the model — a planar laser (height = 1), a tilt laser's sweep, a spinning 3D
 * lidar — as range / geom-id images and point clouds.  A camera cannot stand in for a scanner: a pinhole projection ends below 180
 * degrees, a scan covers 360 of azimuth, and its rows are beam elevations.  The beams are generated on the device from the pattern and
 * the site's pose in each env: no ray buffer is uploaded, and a scanner on a moving body follows it per env.
 *   Beam (i, j) — row i, column j — starts at the site's origin and has, in the sensor frame (+x is azimuth 0, +z the rotation axis,
 *   azimuth counter-clockwise about +z), the direction d = (cos el_i cos az_j, cos el_i sin az_j, sin el_i) with az_j = azimuth0 +
 *   j azimuth_step and el_i = elevation[i], or elevation0 + i elevation_step without a table.  d is a unit vector up to rounding: the
 *   host takes cos / sin of every column azimuth and row elevation in fp64 and rounds each to fp32 once; the device multiplies.
 *   range: the Euclidean distance from the site's origin to the nearest visible surface along the beam; a miss is range -1, geomid -1.
 *   points: range d in the SENSOR frame (what a sensor_msgs/PointCloud2 of the scanner's frame holds); a miss is (0, 0, 0).
 *   Everything else is mjh_ray's on the same engine: the semantics per geom type (a scanner inside a geom sees its far surface),
 *   inactive slots, per-env geom sizes, mjh_ray_set_mesh_mode and mjh_ray_set_mesh_surface, the lower geom id on an exact fp32 tie,
 *   and the call-sequence rules (a pending mjh_step1 goes out first, a window hand-over is dropped).  Nothing of state, statistics,
 *   warm start or time is written.
 *   cull: a wavefront casts a tile of 64 beams (1 x 64 for a planar scan, up to 8 x 8) and walks only the bounded geoms whose
 *   bounding sphere touches the cone over the tile's beams; a tile that spans more than 180 degrees of azimuth gets no cone.
 *   cull = 0 makes every tile visit every geom.  The two give the same bits (the cull may never cost a hit).
 *   The angle tables, 2 (width + height) floats, live in an engine-owned device buffer and are uploaded (in stream order, from an
 *   engine-owned host buffer) only when the pattern differs from the last call's; `elevation` is read during the call only.
 * A site or body id out of range, a non-positive size (or n * width * height of 2^30 or more), an angle that is not finite, a row
 * outside [-pi/2, pi/2], an env range out of bounds or a NULL range pointer return MJH_ERR_ARG and launch nothing. */
typedef struct mjh_scan_options {
  int site;                 /* sensor frame: +x is azimuth 0, +z the rotation axis, azimuth counter-clockwise about +z; -1: world frame */
  int width, height;        /* beams per row (azimuth steps) and rows (elevations); n*width*height below 2^30 */
  double azimuth0, azimuth_step;     /* column j looks at azimuth0 + j*azimuth_step (radians) */
  const double* elevation;           /* [height] radians in [-pi/2, pi/2], any order (real lidars are not uniform); NULL: */
  double elevation0, elevation_step; /*   row i looks at elevation0 + i*elevation_step */
  int bodyexclude, flg_static;       /* as mjh_ray_options */
  int cull;                 /* 1 (default): tile culling; 0: every tile visits every geom -- same bits */
  double cutoff;            /* > 0: a range beyond it is a miss (the scanner's maximum range) */
} mjh_scan_options;
void mjh_scan_default_options(mjh_scan_options*);   /* -1, 360, 1, -pi, 2 pi / 360, NULL, 0, 0, -1, 1, 1, 0: one planar turn in 1-degree steps */
/* device pointers; enqueued on the engine's stream, no synchronisation; d_geomid and d_points may be NULL.  options may be NULL */
int mjh_scan_device(mjh_engine*, int env0, int n, const mjh_scan_options*,
                    float* d_range /*[n][height][width]*/, int* d_geomid /*or NULL*/, float* d_points /*[n][height][width][3] or NULL*/);
/* host pointers (fp32; geomid and points may be NULL): calls the device form through the engine-owned staging buffer and synchronises */
int mjh_scan(mjh_engine*, int env0, int n, const mjh_scan_options*, float* range, int* geomid, float* points);

/* Height scans (elevation maps): a regular height x width grid of PARALLEL rays cast under a site of the model in every env — how high
 * is the terrain under and around a mobile base, turned with its heading but not with its roll and pitch.  Cameras and lidars fan out
 * from one origin; this projection is orthographic.  The rays are generated on the device from the grid and the site's pose in each
 * env: no ray buffer is uploaded, and a sensor on a moving body follows it per env.
 *   Sensor frame: the site's world pose in the env, origin o and rotation S; site = -1 is the world frame.
 *   Grid frame G = (gx, gy, gz), chosen by `align`:
 *     MJH_HSCAN_ALIGN_YAW (default): gz = (0, 0, 1) in the world; gx is the site's x axis projected onto the world's xy-plane and
 *       normalised; gy = gz x gx.  If the squared length of the projection is below 1e-6 (the site's x axis within about 0.06 degrees
 *       of vertical) gx is the world's x axis.  The rays point along the world's -z: roll and pitch of the carrier do not tilt the grid.
 *     MJH_HSCAN_ALIGN_BASE: G = S; the rays point along the site's -z (an orthographic depth camera bolted to the body).
 *     MJH_HSCAN_ALIGN_WORLD: G is the identity; the site supplies the translation only.
 *   Cell (row i, column j) lies in the grid frame at x_j = offset[0] + (j - (width - 1) / 2) spacing[0] and y_i = offset[1] +
 *   (i - (height - 1) / 2) spacing[1]: row 0 is the lowest y, column 0 the lowest x.  Its ray starts at o + gx x_j + gy y_i + gz above
 *   and goes along -gz.
 *   range: the Euclidean distance from the ray's start to the nearest visible surface; a miss is range -1, geomid -1.
 *   points: (x_j, y_i, above - range) in the GRID frame: z is the terrain height relative to the sensor's origin.  A miss takes range 0
 *   in that formula: it is the ray's start point (mjh_scan's rule: a miss is the origin of its beam).
 *   Everything else is mjh_ray's on the same engine: the semantics per geom type (a start point inside a geom sees its far surface),
 *   inactive slots, per-env geom sizes, mjh_ray_set_mesh_mode and mjh_ray_set_mesh_surface, the lower geom id on an exact fp32 tie,
 *   cutoff (applied to range), flg_static, and the call-sequence rules (a pending mjh_step1 goes out first, a window hand-over is
 *   dropped).  Nothing of state, statistics, warm start or time is written.
 *   exclude_tree: 0 (default): bodyexclude hides that one body.  1: every geom whose body has the same body_rootid as bodyexclude is
 *   hidden — the sensor's whole kinematic tree, base, wheels and arm.  The engine uploads the root-id table at the first call that asks.
 *   cull: a wavefront casts a tile of 64 cells (1 x 64 for a single row, up to 8 x 8) and walks only the bounded geoms whose bounding
 *   sphere touches the half-infinite cylinder around the tile's rays.  cull = 0 makes every tile visit every geom.  The two give the
 *   same bits (the cull may never cost a hit).
 * A site or body id out of range, exclude_tree = 1 with bodyexclude < 0, an unknown align, a non-positive size (or n * width * height of
 * 2^30 or more), a spacing that is not finite or not > 0, an offset or `above` that is not finite, a cell coordinate that overflows
 * fp32, an env range out of bounds or a NULL range pointer return MJH_ERR_ARG and launch nothing. */
enum { MJH_HSCAN_ALIGN_YAW = 0, MJH_HSCAN_ALIGN_BASE = 1, MJH_HSCAN_ALIGN_WORLD = 2 };
typedef struct mjh_heightscan_options {
  int site;                 /* sensor frame; -1: the world frame */
  int align;                /* MJH_HSCAN_ALIGN_* */
  int width, height;        /* cells per row (along gx) and rows (along gy); n*width*height below 2^30 */
  double spacing[2];        /* cell pitch along gx and gy, > 0 */
  double offset[2];         /* the grid's centre in the grid frame */
  double above;             /* the rays start this far along +gz */
  int bodyexclude;          /* as mjh_ray_options */
  int exclude_tree;         /* 1: hide every body of bodyexclude's kinematic tree */
  int flg_static;           /* as mjh_ray_options */
  int cull;                 /* 1 (default): tile culling; 0: every tile visits every geom -- same bits */
  double cutoff;            /* > 0: a range beyond it is a miss */
} mjh_heightscan_options;
void mjh_heightscan_default_options(mjh_heightscan_options*);   /* -1, YAW, 16, 16, {0.1, 0.1}, {0, 0}, 1.0, -1, 0, 1, 1, 0 */
/* device pointers; enqueued on the engine's stream, no synchronisation; d_geomid and d_points may be NULL.  options may be NULL */
int mjh_heightscan_device(mjh_engine*, int env0, int n, const mjh_heightscan_options*,
                          float* d_range /*[n][height][width]*/, int* d_geomid /*or NULL*/, float* d_points /*[n][height][width][3] or NULL*/);
/* host pointers (fp32; geomid and points may be NULL): calls the device form through the engine-owned staging buffer and synchronises */
int mjh_heightscan(mjh_engine*, int env0, int n, const mjh_heightscan_options*, float* range, int* geomid, float* points);

/* RGB-D images: beside mjh_depth's depth and geom id, the world-frame surface normal at every pixel's hit and a shaded colour image.
 * Two launches on the engine's stream: the depth launch exactly as mjh_depth_device issues it (so depth and geomid are mjh_depth's
 * bits), then a shading kernel that reads those two images, regenerates each pixel's ray and resolves the normal on the one geom
 * the pixel names.
 *   normal: the unit normal of the surface the ray hits, oriented towards the ray's origin (n . v <= 0: a camera inside a sphere gets
 *   the inward normal of the far surface; two-sided surfaces need no convention); a miss is (0, 0, 0).  In the geom's frame, at the
 *   hit point h, before orientation: plane (0, 0, 1); sphere h / |h|; ellipsoid (h_x / a^2, h_y / b^2, h_z / c^2) normalised; capsule
 *   h - (0, 0, clamp(h_z, -s1, s1)) normalised; cylinder the cap (0, 0, sign h_z) where |h_z| - s1 >= hypot(h_x, h_y) - s0, else radial;
 *   box the axis with the largest |h_i| - s_i, sign of h_i; height field the geometric normal of the top triangle the ray hit, or
 *   the wall's, or the base's; mesh as its hull: the hull plane with the largest n . h - d; mesh as its triangles: e1 x e2 of the
 *   triangle the ray hit.  On an exact tie between two features of one geom (a crease) either feature's normal is right.
 *   rgba: four bytes per pixel, R, G, B, A in memory order.  On a hit channel c of R, G, B is (int)(255 min(1, geom_rgba[g][c] shade)
 *   + 0.5) in fp32 with shade = ambient + diffuse |n . v^| (v^: the unit ray direction), and A is 255: the geom's own alpha is not
 *   used, there is no transparency.  On a miss all four channels are (int)(255 background[c] + 0.5).
 * Any output may be NULL, not all four; with normal and rgba both NULL the call is mjh_depth_device.  Errors are mjh_depth's; in
 * addition ambient or diffuse negative or not finite, or a background component outside [0, 1], return MJH_ERR_ARG.  An error launches
 * nothing and writes nothing.  Call-sequence rules, mesh mode, mesh surface, slot masks, per-env sizes and "nothing of the state is
 * written" are mjh_depth's.  The colour table is uploaded with the other ray tables at the engine's first render call. */
typedef struct mjh_render_options {
  mjh_depth_options view;   /* camera, size, bodyexclude, flg_static, range, cull, cutoff: exactly mjh_depth's */
  float ambient, diffuse;   /* shade = ambient + diffuse * |n . v^|   (defaults 0.3, 0.7: a face-on surface shows its own rgba) */
  float background[4];      /* colour of a miss, components in [0,1] (default 0 0 0 0) */
} mjh_render_options;
void mjh_render_default_options(mjh_render_options*);
/* device pointers; enqueued on the engine's stream, no synchronisation.  An image the caller does not take (NULL) but the shading
 * needs lives in engine-owned scratch.  options may be NULL (the defaults) */
int mjh_render_device(mjh_engine*, int env0, int n, const mjh_render_options*,
                      float* d_depth, int* d_geomid, float* d_normal /*[n][H][W][3]*/, unsigned char* d_rgba /*[n][H][W][4]*/);
/* host pointers: calls the device form through the engine-owned staging buffer and synchronises */
int mjh_render(mjh_engine*, int env0, int n, const mjh_render_options*, float* depth, int* geomid, float* normal, unsigned char* rgba);

/* Lights and cast shadows in the colour image.  mjh_render_set_lighting(engine, mode): 0 (the default) is the call above — the same
 * launches and the same bits whether or not the model has lights; 1: the colour image also takes the model's active lights.  Any other
 * mode returns MJH_ERR_ARG and changes nothing.  Depth, geom id and normal are mode 0's bits in either mode.
 *   Mode 1, a hit on geom g: channel c is level(rgba[g][c] * (shade + sum_l (amb_l[c] + dif_l[c] * t_l))) with shade = ambient +
 *   diffuse |n . v^| as above, level(x) = (int)(255 min(1, x) + 0.5), the sum over the active lights in id order, in fp32; alpha 255;
 *   a miss is the background.  With no active light the launches and the image are mode 0's.
 *   Per light: h = p + x v is the hit point (p the camera origin, v the pixel's ray, x its parameter), n the pixel's normal as the
 *   normal image holds it (towards the camera), L and d^ the light's position and unit direction in the world frame, from its body's
 *   pose in that env.  l = -d^ for a directional light, L - h for a positional one; l^ = l / |l|.
 *     t_l = max(0, n . l^) * spot * lit
 *     spot (positional lights only; 1 for directional ones): with c = -l^ . d^, c^exponent if c >= cos(cutoff), else 0
 *     lit = 0 if options.shadows, the light has castshadow, n . l^ > 0 and the shadow ray is blocked; else 1
 *   The shadow ray starts at o = h + bias n.  Directional light: direction -d^, unbounded.  Positional light: direction L - o, blocked
 *   only by a hit with ray parameter < 1 (a geom beyond the light blocks nothing).  It sees exactly the geoms the image's own rays
 *   see: bodyexclude, flg_static = 0, an inactive slot, mesh mode and mesh surface hide a geom from the shadow ray too, and the view's
 *   cutoff does not bound it.  The pixel's own geom is an occluder like any other (a height field or a torus shadows itself).
 *   Consequences: a surface seen from the side the light is not on (n . l^ <= 0) gets that light's ambient term only; a camera inside
 *   a closed geom sees the inward normal, and every light outside the geom is blocked by it.
 * Launches in mode 1 with an active light and a colour image asked for: the depth launch, unchanged; the shade launch, which writes
 * the normal (into engine-owned scratch if the caller takes none) and no colour; the light kernel on the same stream.
 * The lights are read from the model once, at the engine's first such call; mjh_set_light_active(engine, light, on) switches a light
 * for every env of the engine from the next call on (a bad id: MJH_ERR_ARG).
 * mjh_light_options: shadows 0 casts no shadow ray; cull 0 visits every geom (1: occluders are culled per tile; the bits are the same
 * either way); bias in metres, > 0 and finite.  A shadows or cull value other than 0 / 1, a bad bias or a NULL pointer: MJH_ERR_ARG and
 * nothing changes.  Defaults 1, 1, 1e-3.
 * Not modelled: specular and attenuation terms, soft shadows, per-env light poses in the body frame or colours, moving light
 * modes, lights for mjh_ray. */
typedef struct mjh_light_options { int shadows; int cull; float bias; } mjh_light_options;
void mjh_light_default_options(mjh_light_options*);
int mjh_render_set_lighting(mjh_engine*, int mode);
int mjh_render_get_lighting(const mjh_engine*);
int mjh_render_set_light_options(mjh_engine*, const mjh_light_options*);
int mjh_render_get_light_options(const mjh_engine*, mjh_light_options*);
int mjh_set_light_active(mjh_engine*, int light, int on);

/* Textures in the colour image.  mjh_render_set_texturing(engine, mode): 0 (the default) is the calls above — the same launches and the
 * same bits whether or not the model has textures; 1: where a pixel's geom carries a texture (geom_texid >= 0) its base colour is
 * geom_rgba[g][c] * (t_c / 255) per channel c of R, G, B, with t the texel below; the alpha stays the geom's; everything else (shade,
 * lights, shadows, level()) is as above.  Any other mode returns MJH_ERR_ARG and changes nothing.  Depth, geom id and normal are
 * mode 0's bits in either mode, and so is every pixel whose geom has no texture.
 *   The texel [UPSTREAM, unverified here: MuJoCo's object-linear projection of a 2D texture along the geom's z axis]: with h the hit
 *   point in the geom's frame, X = h_x / a_x, Y = h_y / a_y, where a = (1, 1) if geom_texuniform, else the geom's half extents in x
 *   and y from the env's size row: plane size[0..1] (a component of 0, an infinite plane, counts as 1), box and ellipsoid
 *   size[0..1], sphere, capsule and cylinder (r, r), height field hfield_size[0..1].  u = 0.5 rx X + 0.5, v = 0.5 - 0.5 ry Y with
 *   (rx, ry) = geom_texrepeat; column i = min(W-1, floor((u - floor u) W)), row j the same from v and H.  Nearest texel, in fp32: no
 *   filtering, no mip levels.  The sides of a box show the texture stretched along z.
 * Launches in mode 1 with a colour image asked for and ntex > 0: the depth launch, unchanged; the texture kernel, which writes one
 * word per pixel (R, G, B, flag) into engine-owned scratch; the shade launch; the light kernel (lighting mode 1 only).  The textures
 * are uploaded once per engine, at its first such call.
 * Not modelled: file, cube and skybox textures, mark="random", textures on mesh geoms, per-env textures, reflectance / specular /
 * emission. */
int mjh_render_set_texturing(mjh_engine*, int mode);
int mjh_render_get_texturing(const mjh_engine*);

/* zero-copy export for the single ROS state topic: packs time(1)+qpos(nq)+qvel(nv)
 * fp32 per env into a caller-provided DEVICE buffer [nenv*(1+nq+nv)] on the engine's
 * stream (feeds the RCCL all-gather). */
int mjh_export_state_device(mjh_engine*, void* d_out);
int mjh_state_stride(const mjh_engine*);

/* Pinned host mirror of envs [env0, env0+n) for the publisher threads: the reference's ROS layer
 * reads d->qpos / qvel / qfrc_inverse (joint states, mj_ros.cpp:2164-2194), d->xpos / xquat (tf, object states,
 * :2096-2149) and d->geom_xpos / geom_xmat (markers, :1968-2094) at each topic's own rate.  mjh_mirror_update() enqueues
 * an asynchronous refresh of the selected parts behind the steps queued so far and returns at once; mjh_mirror_wait()
 * blocks until the latest refresh has landed; mjh_mirror_field() returns the fp32 rows (env-major, `row_width` floats per
 * env) inside the pinned block. */
typedef struct mjh_mirror mjh_mirror;
enum { MJH_MIRROR_JOINTS = 1, MJH_MIRROR_BODIES = 2, MJH_MIRROR_GEOMS = 4 };
enum { MJH_MIRROR_TIME = 0, MJH_MIRROR_QPOS = 1, MJH_MIRROR_QVEL = 2, MJH_MIRROR_QFRC_INVERSE = 3, MJH_MIRROR_XPOS = 4,
       MJH_MIRROR_XQUAT = 5, MJH_MIRROR_GEOM_XPOS = 6, MJH_MIRROR_GEOM_XMAT = 7 };
int mjh_mirror_create(mjh_engine*, int env0, int n, mjh_mirror** out);
void mjh_mirror_destroy(mjh_mirror*);
int mjh_mirror_update(mjh_mirror*, int what);
int mjh_mirror_wait(mjh_mirror*);
const float* mjh_mirror_field(const mjh_mirror*, int which, int* row_width);
/* the mirrored simulation time of the n environments in fp64 (field MJH_MIRROR_TIME holds the same doubles: row_width 2 floats) */
const double* mjh_mirror_time(const mjh_mirror*);

/* debug: mean shader-clock ticks from kernel start to each of the 16 stage boundaries of one fused step
   (with_inverse bit 3, window-chain models: of the assemble-only launch alone; a -DMJH_COLLIDE_PROBE library also fills out[16 .. 18],
   so callers of that form pass 20 doubles) */
int mjh_debug_stage_cycles(mjh_engine*, int with_inverse, double* out16);
/* debug: raw stamps of one step launch, out[nenv*20] indexed by launch position: [0..15] shader-clock stage stamps,
 * [16],[17] 100 MHz wall clock at start/end, [18] HW_ID | XCC_ID<<32, [19] env id (tools/timeline.py) */
int mjh_debug_stage_raw(mjh_engine*, int with_inverse, long long* out);
/* debug: the solve launch of a free-body model's many-body chain (C2) timed on the pools of the last step — out_ms[0] as it is,
 * out_ms[1] with every wave reading the block operands of one of `slices` environments (an L2-resident working set): what the
 * operand stream from MALL / HBM costs the sweeps.  out_iter[2]: mean sweeps of the two runs. */
int mjh_debug_solve_probe(mjh_engine*, int slices, int reps, double* out_ms, double* out_iter);
/* debug: one step launch that returns at stage boundary `stage` (1..14) and stores nothing (tools/stage_valu.sh:
 * per-stage hardware-counter differences) */
int mjh_debug_stop_at(mjh_engine*, int stage, int with_inverse);

/* ---- launch scheduling (no reference counterpart: the reference steps one mjData on one CPU thread,
 * mj_main.cpp:82-112).  Environments are independent, so mjh_step() may split them into `n` cohorts
 * (contiguous env ranges, 1..8), each stepped on its own HIP stream: the low-occupancy tail of one cohort's
 * step kernel then overlaps the bulk of another's, across consecutive mjh_step calls too.  The split entry
 * points of the reference's loop (mjh_step1 / mjh_inverse / mjh_step2) are issued per cohort as well, and the
 * two calls that loop makes for ONE robot in between — mjh_get_joint_state and mjh_set_cmd (MjHWInterface::read /
 * write) — on an env range inside one cohort are ordered on that cohort's stream only: the host waits for that
 * cohort, the others keep stepping.  The caller's stream forks into the cohort streams inside these calls and is
 * joined again by the next call of any other entry point (and by a ranged call that spans cohorts), so results and
 * ordering seen through this API do not depend on `n` (tests/test_gpu_round3.py: bitwise).  Within a launch the
 * envs are dispatched longest-solver-job first (order rebuilt on the device every MJH_ORDER_EVERY-th step, default 8).
 * Default n: 1 below 1024 envs, else 2 for the fused step and 3 (from 1536 envs) for the three-launch step of the many-body layout
 * (MJH_COHORTS overrides it for engines created afterwards). */
/* m->opt.timestep of a running engine: simulate() doubles it while the simulation lags the wall clock by > 1 ms (up to
 * max_time_step) and halves it back otherwise (mj_main.cpp:150-163) */
int mjh_set_timestep(mjh_engine*, double dt);
double mjh_get_timestep(const mjh_engine*);

/* Memory layout of engines created afterwards (process-wide; no reference counterpart).  0 (default): per-env
 * contact / block / Jacobian pools in LDS while they are small (<= 24 KB per env), otherwise in a per-env slice of global
 * memory with the step issued as three launches (assemble, solve, integrate); 1: LDS whenever the working set fits one
 * CU's 160 KiB; 2: global pools whenever possible.  Results do not depend on the layout beyond fp32 rounding. */
void mjh_set_layout_policy(int policy);
/* Engines created afterwards (process-wide; default 1, environment MJH_WINDOW): mjh_step of a small free-body model (the models that take
 * the contact-patch sweep: every kinematic tree a single free body, nv <= 32) in the default row order runs as two launches — the step
 * kernel up to the constraint rows, then mjh_window_kernel (csrc/window_pgs.h): projected Gauss-Seidel over windows of 16 consecutive
 * rows, FOUR environments per wavefront with the rows in registers, followed by mj_Euler.  0: the one-launch fused step with the
 * contact-patch sweep (same order, same iterates up to fp32 rounding).  mjh_window_solver() reports what an engine runs. */
void mjh_set_window_solver(int on);
int mjh_window_solver(const mjh_engine*);

/* ---- contact report: which bodies touch what, and with how much force, for every env, on the device.
 * mjh_set_contact_report(on): engines created afterwards (process-wide; default 0, environment MJH_CONTACT_REPORT).  Off is the engine as
 * it is without this section: the same layouts, kernel instances, launches and bits.  On, every launch that takes the solve to its end
 * (mjh_step, mjh_step2, mjh_forward) leaves per env, in fp32, the report of its LAST solve (as sensordata):
 *   ncon; one record of 20 words per contact of the collision stage, in its order — dist, pos[3], frame[9], force[4], geom1, geom2, dim
 *   (three ints) —; cfrc_ext[6 * nbody].
 *   force: normal, tangent 1, tangent 2, torque about the normal, in the contact frame, ON geom2's body (mj_contactForce for condim <= 4;
 *   condim 6 does not exist here).  A contact that got no constraint rows (row capacity) is listed with zero force.
 *   cfrc_ext: d->cfrc_ext — torque(3) then force(3) per body, world axes, about the subtree COM of the body's tree root; body 0 is zero;
 *   it sums xfrc_applied, the contact forces and the connect / weld forces.
 * The price: such an engine lays its model out as a model with a force sensor — everything the report reads stays alive after the solve,
 * no diagonal-M form, no contact-patch sweep, no window chain, the many-body layout steps in one fused launch (DESIGN.md section 4h has the
 * figures).  Results agree with a report-off engine to fp32 rounding, as with every layout choice.
 * Every function below returns MJH_ERR_STATE on an engine created with the report off.  Before the first solve, and for an env after
 * mjh_reset, the report is ncon = 0 and zeros.  Not forwarded by mjh_group, not part of the pinned mirror. */
void mjh_set_contact_report(int on);
int mjh_contact_report(const mjh_engine*);   /* what this engine does; NULL: the switch, i.e. what an engine created now would do */
/* the engine's device buffers: int ncon[nenv], float records[nenv][maxcon][20], float cfrc_ext[nenv][6 * nbody]; valid until mjh_destroy,
 * they hold the report of the last solve once the engine's stream has reached it.  Any output may be NULL. */
int mjh_contact_report_device(mjh_engine*, const void** d_ncon, const void** d_records, const void** d_cfrc_ext, int* maxcon);
/* host copies (synchronise): ncon [n]; per env maxcon slots of dist [1], pos [3], frame [9], force [6] (mj_contactForce's layout: entries 4
 * and 5 are zero), geom [2], dim [1]; slots from ncon on are zero.  Any output may be NULL. */
int mjh_get_contact_forces(mjh_engine*, int env0, int n, int* ncon, double* dist, double* pos, double* frame, double* force, int* geom, int* dim);
int mjh_get_cfrc_ext(mjh_engine*, int env0, int n, double* cfrc_ext /* [n * 6 * nbody] */);
/* Net contact force ON selected bodies, world axes: force[i][s] = sum over env env0 + i's contacts that touch body[s] (+ the record's force
 * where the body carries geom2, - where it carries geom1), restricted to contacts whose other body is against[s] unless that is -1
 * (against NULL: all -1); count[i][s] = contacts that entered the sum.  One launch of mjh_contact_force_kernel (csrc/contact.hip) on the
 * engine's stream behind the steps queued so far; the selection table is uploaded only when it differs from the last call's.  The order
 * of the additions is fixed per env and body: a sum does not depend on nenv, env0, n or the other selected bodies (bitwise).
 * A contact between two selected bodies enters both sums with opposite signs.  Device form: d_force float [n][nsel][3], d_count int
 * [n][nsel] or NULL, no synchronisation.  Host form: doubles, synchronises; count may be NULL.
 * An env range out of bounds, nsel <= 0, a body id outside [0, nbody), an `against` outside [-1, nbody) or a NULL force pointer return
 * MJH_ERR_ARG and launch nothing; a contact capacity beyond 3276 (the kernel's LDS stage) MJH_ERR_CAPACITY. */
int mjh_body_contact_force_device(mjh_engine*, int env0, int n, int nsel, const int* body, const int* against, void* d_force, void* d_count);
int mjh_body_contact_force(mjh_engine*, int env0, int n, int nsel, const int* body, const int* against, double* force, int* count);
/* ------------------------------------------------- frame states: pose, twist and Jacobian of bodies and sites
 * What the robot is doing in Cartesian terms, for every env, without a host round trip.  A frame is (objtype, id); its world pose is
 *   body: xpos[b], xquat[b];   site: xpos[b] + R_b site_pos, xquat[b] * site_quat with b = site_bodyid.
 * Jacobian (world axes, at the frame's world origin p; mj_jacBody / mj_jacSite): one column per dof of the frame's body and of its
 * ancestors, every other column zero —
 *   slide: jacp = axis, jacr = 0;   hinge: jacr = axis, jacp = axis x (p - anchor);
 *   free joint: three translational columns with the world unit axes, then three rotational columns with the BODY's axes through xpos[b];
 *   ball: three rotational columns with the body's axes (after the ball's rotation) through the joint anchor;
 * axis and anchor of a joint taken with the body frame as it stands after the body's joints before it (mj_kinematics' order).
 * Twist: linvel = jacp qvel, angvel = jacr qvel (mj_objectVelocity with flg_local = 0, the linear part first).
 * Per frame: flags & MJH_FRAME_LOCAL rotates the twist into the frame's own axes (velocimeter / gyro; the pose stays the world pose);
 * refid >= 0 reports pose and twist relative to the frame (reftype, refid), in its axes (MuJoCo's frame sensors with reftype):
 *   pos = Rr^T (p - pr), quat = qr^-1 q, linvel = Rr^T (v - vr - wr x (p - pr)), angvel = Rr^T (w - wr);   refid = -1: no ref.
 * Output per env and frame, 13 numbers: pos[3], quat[4] (w first), linvel[3], angvel[3].  The Jacobian is optional: [n][nframe][6][nv],
 * rows 0-2 jacp, rows 3-5 jacr, always in world axes at the frame's world origin, whatever ref / LOCAL say.
 * Poses and velocities are those of the envs' present qpos / qvel (after mjh_step: the state at the new time).  A mocap body reports the
 * pose set per env, zero twist and a zero Jacobian; bodies of inactive slots are reported as they are.
 * One position-stage launch of the env range (as mjh_get_body_state issues it) and one launch of mjh_frame_state_kernel (csrc/frame.hip) on
 * the engine's stream behind the steps queued so far; nothing of the envs' state, statistics or time is written.  The frame table is
 * uploaded only when it differs from the last call's; the per-model tables are built at the first call.  The order of the additions is
 * fixed per env and frame: a result does not depend on nenv, env0, n, the other frames of the call or on whether a Jacobian was asked
 * for (bitwise).  Device form: d_state float [n][nframe][13], d_jac float [n][nframe][6][nv] or NULL, no synchronisation.  Host form:
 * doubles, synchronises; jac may be NULL.
 * An env range out of bounds, nframe <= 0, an objtype other than 0 / 1, an id outside [0, nbody) / [0, nsite), a bad ref, LOCAL together
 * with a ref, a NULL frames / state pointer, or n * nframe * 6 * nv beyond 2^30 with a Jacobian return MJH_ERR_ARG and launch nothing; an
 * nv beyond 2048 (the kernel's LDS stage of 8 words per dof) MJH_ERR_CAPACITY.  Not forwarded by mjh_group, not part of the pinned mirror. */
enum { MJH_FRAME_BODY = 0, MJH_FRAME_SITE = 1 };
enum { MJH_FRAME_LOCAL = 1 };
typedef struct mjh_frame { int objtype, id, reftype, refid, flags; } mjh_frame;
int mjh_frame_state_device(mjh_engine*, int env0, int n, int nframe, const mjh_frame* frames, void* d_state, void* d_jac);
int mjh_frame_state(mjh_engine*, int env0, int n, int nframe, const mjh_frame* frames, double* state, double* jac);
/* ------------------------------------------------- frame accelerations: IMU accelerometer readings and Jdot qvel of bodies and sites
 * Per env and frame, with p the frame's world origin carried by its body and J(p) the Jacobian of mjh_frame_state:
 *   acc  = linacc[3], angacc[3] = J(p) qacc + Jdot(p) qvel: the classical acceleration d2p/dt2 of the point and the angular acceleration of
 *          the body, in world axes.  flags & MJH_FRAME_PROPER subtracts the model's gravity from linacc (a body at rest reads -g, a body
 *          in free fall 0: MuJoCo's cacc[world] = -gravity convention; nothing is subtracted with MJH_DSBL_GRAVITY); flags &
 *          MJH_FRAME_LOCAL then rotates both vectors into the frame's own axes.  LOCAL | PROPER on a site is MuJoCo's <accelerometer>
 *          (LOCAL on mjh_frame_state stays the <gyro> and the <velocimeter>).
 *   bias = Jdot(p) qvel, the linear part first, without the qacc term: always in world axes at the frame's world origin whatever the flags
 *          say, as the Jacobian output of mjh_frame_state is — with that Jacobian what a task-space controller needs.  Optional.
 * refid must be -1: acceleration has no ref-relative form here.  MJH_FRAME_PROPER is valid in these two calls only.
 * The call reads the envs' present qpos and qvel and the engine's qacc array, that is the qacc of the last solve (mjh_get_field "qacc");
 * the warm start of mjh_set_state writes the same array.  Timing: after mjh_forward the three are one consistent state and the result is
 * exact; after mjh_step pose and velocity are at the new time and qacc is that of the step just taken — MuJoCo's own one-step staleness of
 * sensordata, first-order accurate in the timestep.  Nothing of the envs' state, statistics or time is written.
 * A mocap body and the world report zero acceleration (-g with PROPER) and a zero bias; bodies of inactive slots are reported as they are.
 * One position-stage launch of the env range and one launch of mjh_frame_accel_kernel (csrc/frame_acc.hip) on the engine's stream behind
 * the steps queued so far, as mjh_frame_state; the frame table (kept apart from mjh_frame_state's: alternating calls upload nothing) is
 * uploaded only when it differs from the last accel call's.  The order of the additions is fixed per env and frame: a result does not
 * depend on nenv, env0, n, the other frames of the call or on whether the bias was asked for (bitwise).  Device form: d_acc float
 * [n][nframe][6], d_bias float [n][nframe][6] or NULL, no synchronisation.  Host form: doubles, synchronises; bias may be NULL.
 * An env range out of bounds, nframe <= 0, an objtype other than 0 / 1, an id outside [0, nbody) / [0, nsite), refid >= 0 (or < -1), a
 * flag outside LOCAL | PROPER, a NULL frames / acc pointer, or n * nframe * 6 beyond 2^30 return MJH_ERR_ARG and launch nothing; an nv
 * beyond 1092 (the kernel's LDS stage of 15 words per dof within the 64 KiB a launch gets without raising its dynamic-LDS limit)
 * MJH_ERR_CAPACITY.  Not forwarded by mjh_group, not part of the pinned mirror. */
enum { MJH_FRAME_PROPER = 2 };   /* beside MJH_FRAME_LOCAL = 1; valid in the two calls below only */
int mjh_frame_accel_device(mjh_engine*, int env0, int n, int nframe, const mjh_frame* frames, void* d_acc, void* d_bias);
int mjh_frame_accel(mjh_engine*, int env0, int n, int nframe, const mjh_frame* frames, double* acc, double* bias);
int mjh_set_cohorts(mjh_engine*, int n);
int mjh_get_cohorts(const mjh_engine*);
/* mjh_step(e, n) of an articulated model in the LDS-resident layout runs up to `n` steps per launch and cohort with the environment's
 * state resident in LDS between them (the in-kernel step loop; default 8, 1 = one launch per step; bitwise the same results).
 * mjh_get_steps_per_launch: what the engine's mjh_step uses — 1 for free-body models and the many-body chain, whose steps are
 * chains of launches (src/mj_main.cpp:83-108 is one step of ONE world; the batch steps n times before the host looks again). */
int mjh_set_steps_per_launch(mjh_engine*, int n);
int mjh_get_steps_per_launch(const mjh_engine*);
/* Launch chains as graphs.  Where a step is a chain of launches per cohort — the window chain of small free-body models (assemble ->
 * window kernel) and the many-body layout (assemble -> [dense build -> dense solve] -> solve -> integrate) — mjh_step captures the
 * chain once per cohort and variant (hipStreamBeginCapture on the cohort's stream) and queues every further cohort-step with ONE
 * hipGraphLaunch; the graph is captured again whenever something its kernels take by value changes.  Same kernels, same arguments, same
 * order: results are bitwise those of the separate launches.  mode (also MJH_CHAIN_GRAPH): 1 (default) the many-body chain only, 2 the
 * window chain as well (measured slower on S24: two plain launches stay the default there), 0 every launch on its own.
 * mjh_launches_per_step: queue entries the LAST mjh_step issued per cohort-step — 1 when it replayed a captured graph, else the chain's
 * kernel launches (2 window chain, 3 / 5 many-body block / dense chain, 1 fused kernel): plain launches are also what a step falls back to
 * on the NULL stream, on a stream that is already being captured and after a failed capture / instantiate (latched per cohort and variant).
 * Before the first step (and after mjh_set_cohorts): what the next step intends.  A retired graph exec is destroyed only after the
 * stream it was last launched on has drained. */
void mjh_set_chain_graph(int mode);
int mjh_launches_per_step(const mjh_engine*);
/* HIP-event timing of the step-kernel launches on the stream they run on: enable (on = 1: every launch, on = N > 1: every
 * N-th launch — the event pairs cost stream time of their own, visible in launch-bound configs), step, then read the mean
 * duration [ms] and the number of launches timed since the last read (bench.py's roofline leg). */
int mjh_set_launch_timing(mjh_engine*, int on);
int mjh_get_launch_timing(mjh_engine*, double* mean_ms, int* count);

/* ---- multi-GPU: the environments of ONE simulation sharded over the GPUs of a node, driven by ONE host thread.
 * The reference is a single C++ node with a single publisher set (src/mj_main.cpp:167-236, src/mujoco_sim/mj_ros.cpp:554-564).
 * Environments are independent, so a group is one engine + one stream per device over contiguous env ranges
 * [k*N/G + min(k, N%G), ...) (shares differ by at most one), model tables replicated and NO collective in the step; the only
 * exchange is mjh_group_publish(): every device packs its slice (time | qpos | qvel per env, fp32, mjh_export_state_device)
 * and one RCCL ncclAllGather over xGMI leaves the full env-ordered state on EVERY device — issued at the state topic's rate,
 * not per step.  RCCL is resolved at run time (dlopen); without it, or when a device is listed twice, the
 * gather uses peer copies.  Everything else (commands, getters, slots, mirrors) goes through the per-device engines with
 * LOCAL env ids: mjh_group_engine() / mjh_group_locate().  All calls are asynchronous like their mjh_* counterparts. */
typedef struct mjh_group mjh_group;
int mjh_group_create(const mjh_model* model, int nenv_total, const int* devices /* NULL: 0..ndev-1 */, int ndev, mjh_group** out);
void mjh_group_destroy(mjh_group*);
int mjh_group_ndev(const mjh_group*);
int mjh_group_nenv(const mjh_group*);
mjh_engine* mjh_group_engine(mjh_group*, int rank);
int mjh_group_env_range(const mjh_group*, int rank, int* env0, int* n);
int mjh_group_locate(const mjh_group*, int env, int* rank, int* local_env);
int mjh_group_step(mjh_group*, int nsteps, int with_inverse);   /* mjh_step on every device */
int mjh_group_step1(mjh_group*);                                /* mj_main.cpp:83 on every device */
int mjh_group_inverse(mjh_group*);
int mjh_group_step2(mjh_group*);                                /* mj_main.cpp:108 */
int mjh_group_reset(mjh_group*);
int mjh_group_synchronize(mjh_group*);
/* pack + all-gather; host_out (may be NULL) receives device 0's copy: [nenv_total * mjh_group_state_stride()] floats, env order */
int mjh_group_publish(mjh_group*, float* host_out);
/* the gathered state on device `rank`: valid once the publish's exchange — which runs on a communication stream of its own,
 * beside the steps — has finished: after mjh_group_wait_publish(rank, stream) in that stream's order, after
 * mjh_group_synchronize(), or after a publish with host_out */
const float* mjh_group_state_device(const mjh_group*, int rank);
int mjh_group_wait_publish(mjh_group*, int rank, void* stream /* NULL: the device's engine stream */);
/* ... and the consumer's release: `stream` has finished reading the gathered state of device `rank` up to this point of its order.
 * The NEXT publish overwrites that buffer; its exchange waits for the release.  A consumer that reads asynchronously without
 * releasing must synchronise before the next mjh_group_publish. */
int mjh_group_release_publish(mjh_group*, int rank, void* stream /* NULL: the device's engine stream */);
int mjh_group_state_stride(const mjh_group*);
int mjh_group_uses_rccl(const mjh_group*);
/* HIP events on device 0's COMMUNICATION stream around the exchange of every publish (the all-gather, or the peer copies): mean duration in
 * milliseconds and the number of publishes since the last call */
int mjh_group_set_publish_timing(mjh_group*, int on);
int mjh_group_get_publish_timing(mjh_group*, double* mean_ms, int* count);
void mjh_group_set_transport(int mode);   /* groups created afterwards: 0 = RCCL when available and the devices are distinct (default), 1 = peer copies,
                                             2 = RCCL also when a device is listed twice (a real RCCL refuses that at ncclCommInitAll and the group falls back to peer
                                             copies; the recording stand-in of tests/nccl_stub, named by MJH_RCCL_LIB, accepts it: N ranks on one device) */
/* Test hook, no device needed: the RCCL call sequence of `publishes` exchanges with `ndev` ranks exactly as mjh_group_publish issues it
 * (per_thread != 0: a host thread per rank enqueues its own ncclAllGather; 0: one grouped call inside ncclGroupStart / ncclGroupEnd), between
 * ncclCommInitAll and ncclCommDestroy, against the library MJH_RCCL_LIB names (default: the process's RCCL); buffers and streams are
 * made-up addresses that are only passed through. */
int mjh_debug_rccl_exchange(int ndev, int per_thread, unsigned long slot_floats, int publishes);
/* Host threads of a group (groups created afterwards; default 1, environment MJH_GROUP_THREADS): 1 = one persistent host thread per device
 * issues that device's launches, exports and its rank of the all-gather, every mjh_group_* call posts one job per device and waits for
 * them — the host time of a call is that of ONE device (the reference steps on one thread, mj_main.cpp:203: with eight devices behind
 * it that thread's launch calls alone would be as long as a light scene's step); 0 = the caller's thread issues everything, one device
 * after the other.  Same launches in the same per-device order either way: results are bitwise the same.  mjh_group_host_threads:
 * the number of such threads of a group (0: none). */
void mjh_group_set_host_threads(int on);
int mjh_group_host_threads(const mjh_group* g);

/* ROS-free harness of the host loop (csrc/host_sim.cpp: simulate() + MjhHWInterface, mirrors of
 * mj_main.cpp:76-164 and mj_hw_interface.cpp:59-110) with an in-process PD effort controller on
 * every hinge/slide joint of env `env`; returns final joint positions / efforts and the real-time factor */
int mjh_host_run_pd(mjh_engine*, int env, const double* target, double kp, double kd, long nsteps,
                    double* out_qpos, double* out_effort, double* out_rtf);

/* the same harness over a multi-GPU group: the ROS surface attached to GLOBAL env `env`, every shard stepped each step
 * (mjh_group_step1 / inverse / step2), the state slice of all environments all-gathered every `publish_every` steps; out_state
 * (may be NULL, [nenv_total * stride] floats) receives the last published slice */
int mjh_host_run_pd_group(mjh_group*, int env, const double* target, double kp, double kd, long nsteps, int publish_every,
                          double* out_qpos, double* out_effort, float* out_state);
/* simulate() with its real-time pacing switched ON (mj_main.cpp:115-163): the wall-clock spin that holds the real-time factor
 * at <= 1 and the adaptive timestep (doubled while the simulation lags the wall clock by > 1 ms, up to max_time_step; halved
 * back otherwise).  out_stats6 = {sim_time, wall_time, rtf, final_dt, steps, dt_changes} */
int mjh_host_run_realtime(mjh_engine*, int env, const double* target, double kp, double kd, long nsteps, double max_time_step,
                          double* out_stats6);

/* introspection */
int mjh_nenv(const mjh_engine*);
const mjh_model* mjh_engine_model(const mjh_engine*);
int mjh_lds_bytes(const mjh_engine*);  /* dynamic LDS per env (= per workgroup) */
/* Gauss-Seidel visiting order of the engine's solver sweeps: 2 = the constraint rows of efc_* in their own order, the order
 * mj_solPGS (engine_solver.c, reached through mj_step2, mj_main.cpp:108) walks — the DEFAULT; 1 / 0 = the legacy orders that regroup
 * the rows to expose more independent work (1: contact patches sorted by body pair, small free-body models; 0: independent pairs /
 * groups of constraint blocks).  Any order is a valid PGS iteration and they agree at convergence; stopped at the iteration cap they do
 * not (BASELINE.md section 3 has the size of that effect), which is why the reference's order is the default. */
int mjh_solver_order(const mjh_engine*);
/* How the engine walks that order: 1 = row order with a precedence-preserving list schedule (default) — a constraint block (or contact
 * patch) starts once every EARLIER block that shares a kinematic tree with it is done; blocks without a common tree touch disjoint
 * dofs, their updates commute exactly, so up to 2 / 4 / 16 of them run side by side in one wavefront and the iterates (and the sweep
 * count: the convergence test sums fixed-point integers) are bit-identical to the strictly sequential sweep; 2 = that sequential sweep
 * itself, one block after the other (the reference the tests compare 1 against); 0 = a legacy reordering schedule (mjh_solver_order
 * says which). */
int mjh_pgs_schedule(const mjh_engine*);
/* 1: the engine's sweeps take the contact-patch form (csrc/patch_pgs.h: small free-body models — up to 16 rows between the same two
 * bodies are one unit, up to four units side by side), 0: a block form (one constraint block = one equality / limit / friction-loss
 * row or the pyramid rows of one contact) */
int mjh_patch_sweep(const mjh_engine*);
/* Gauss-Seidel order / schedule of engines created afterwards (process-wide; no reference counterpart): 1 (default), 2 or 0 as
 * mjh_pgs_schedule reports them.  Articulated models whose sweeps are sequential in any case (more than 32 dofs and a kinematic tree
 * of more than 16) run row order under 0 as well. */
void mjh_set_pgs_row_order(int mode);
/* 1: mjh_step solves the environments of this engine whose rows fit with the dense row-space solver (AR = J M^-1 J^T on the matrix
 * cores, column sweeps: csrc/dense_pgs.h) — articulated models in the many-body layout; same rows, same visiting order, same results up
 * to fp32 rounding as the block solver (MJH_DENSE=0 turns it off) */
int mjh_dense_solver(const mjh_engine*);
int mjh_query_lds_bytes(const mjh_model*); /* same figure without a device: capacity planning (160 KiB per CU) */
int mjh_debug_lds_layout(const mjh_model*, char* out, int cap);   /* the LDS layout as text ("name offset" per array, float units; then totals): capacity planning, tools/lds_layout.py */
int mjh_query_lds_bytes_assemble(const mjh_model*);   /* LDS per env of the assemble-only launch of the window chain (small free-body models; 0: not taken); models within 64 contacts: that launch's extent in the fused layout's offsets, an upper bound — what it allocates is `lds_bytes_wpre` of mjh_debug_lds_layout */
const char* mjh_last_error(void);
const char* mjh_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MJHIP_H_ */
