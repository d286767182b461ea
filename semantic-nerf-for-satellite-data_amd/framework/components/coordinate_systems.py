"""Coordinate systems of the scene loaders (the reference's framework/components/coordinate_systems.py offers a custom ECEF
system and a UTM one).  Only the custom ECEF system is built, and its conversions run on the device inside the ray and
reprojection kernels (csrc/satrays.hip: latlon_to_ecef, ecef_to_latlon); the package holds no host copy of them.  The UTM
system needs utm / pyproj, which this build does not carry: asking for it is an error, not a silent switch to ECEF."""

CUSTOM_ECEF = "custom_ecef"


def init_coordinate_system(cfgs) -> str:
    """the datasets' coordinate system: CUSTOM_ECEF, or an error for `use_utm_coordinate_system`"""
    if getattr(cfgs.pipeline, "use_utm_coordinate_system", False):
        raise NotImplementedError("use_utm_coordinate_system = true: the UTM coordinate system needs the utm / pyproj packages, "
                                  "which this build does not carry; scenes load in the custom ECEF system only")
    return CUSTOM_ECEF
