// surface_tex_steps.inc — the steps of the textured resolve that more than one kernel takes, as the lines themselves: included by
// resolve_textured_surfaces_kernel (surface_tex_kernel.h), which is compiled from the lines it always had, and by
// shade_channels_kernel (channel_kernel.h), with MRT_TEX_STEP naming the step.  (A shared __device__ function in their place changes
// the resolve's machine code: DESIGN.md 4.21.)  The including kernel provides, by these names: s (n_tris, n_materials, present,
// shade_rows), t (TextureParams), prim, u, v, and from step 2 on w = (1 - u) - v; o3.x / o3.y receive the UV; nx, ny, nz hold the
// record's normal before step 3, the smooth normal after it and the perturbed normal after step 5.
#if MRT_TEX_STEP == 1 // in_range and the 64-byte shade row
		const bool in_range = prim < s.n_tris;
		float4 t0 = {}, t1 = {}, t2 = {}, t3 = {};
		if (in_range && s.present != 0u) {
			const float4 *row = reinterpret_cast<const float4 *>(s.shade_rows) + (size_t)prim * 4u;
			t0 = row[0]; t1 = row[1]; t2 = row[2]; t3 = row[3];
		}
#elif MRT_TEX_STEP == 2 // uv and uv_ok
		bool uv_ok = false;
		if (in_range && (s.present & SHADE_HAS_UVS)) {
			o3.x = (t1.w * w + t3.x * u) + t3.z * v;
			o3.y = (t2.w * w + t3.y * u) + t3.w * v;
			uv_ok = fabsf(o3.x) < __builtin_inff() && fabsf(o3.y) < __builtin_inff(); // (false for a NaN)
		}
#elif MRT_TEX_STEP == 3 // the smooth normal
		if (in_range && (s.present & SHADE_HAS_NORMALS)) {
			nx = (t0.x * w + t1.x * u) + t2.x * v;
			ny = (t0.y * w + t1.y * u) + t2.y * v;
			nz = (t0.z * w + t1.z * u) + t2.z * v;
			normalize3(nx, ny, nz);
		}
#elif MRT_TEX_STEP == 4 // the material's binding
		const uint32_t id = __float_as_uint(t0.w);
		const bool material = in_range && (s.present & SHADE_HAS_IDS) && id < s.n_materials;
		uint32_t albedo_tex = MRT_NO_TEXTURE, normal_tex = MRT_NO_TEXTURE;
		float normal_scale = 0.0f;
		if (material && id < t.n_bindings) {
			const uint4 b = reinterpret_cast<const uint4 *>(t.bindings)[id];
			albedo_tex = b.x; normal_tex = b.y; normal_scale = __uint_as_float(b.z);
		}
#elif MRT_TEX_STEP == 5 // perturb_normal, where the binding's normal map applies
		if (normal_tex != MRT_NO_TEXTURE && t.tangents != nullptr && prim < t.n_tangent_tris && uv_ok) {
			const float4 *tr = reinterpret_cast<const float4 *>(t.tangents) + (size_t)prim * 3u;
			const float4 a0 = tr[0], a1 = tr[1], a2 = tr[2]; // {t0 xyz, t1.x | t1 yz, t2 xy | t2.z, sign0, sign1, sign2}
			if (a2.y != 0.0f || a2.z != 0.0f || a2.w != 0.0f) {
				float tx = (a0.x * w + a0.w * u) + a1.z * v;
				float ty = (a0.y * w + a1.x * u) + a1.w * v;
				float tz = (a0.z * w + a1.y * u) + a2.x * v;
				const float tl2 = (tx * tx + ty * ty) + tz * tz;
				if (tl2 < 1e-8f) { tx = 1.0f; ty = 0.0f; tz = 0.0f; }
				else { const float l = sqrtf(tl2); tx = tx / l; ty = ty / l; tz = tz / l; }
				const float bsign = ((a2.y * w + a2.z * u) + a2.w * v) >= 0.0f ? 1.0f : -1.0f;
				const float k = (nx * tx + ny * ty) + nz * tz;
				tx = tx - nx * k; ty = ty - ny * k; tz = tz - nz * k;
				normalize3(tx, ty, tz);
				const float bx = (ny * tz - nz * ty) * bsign, by = (nz * tx - nx * tz) * bsign, bz = (nx * ty - ny * tx) * bsign;
				float cr, cg, cb;
				sample_bilinear(t, normal_tex, o3.x, o3.y, cr, cg, cb);
				float sx = cr * 2.0f - 1.0f, sy = cg * 2.0f - 1.0f;
				const float sz = cb * 2.0f - 1.0f;
				sx = sx * normal_scale; sy = sy * normal_scale;
				const float px = (tx * sx + bx * sy) + nx * sz, py = (ty * sx + by * sy) + ny * sz, pz = (tz * sx + bz * sy) + nz * sz;
				const float pl2 = (px * px + py * py) + pz * pz;
				if (!(pl2 < 1e-8f)) { const float l = sqrtf(pl2); nx = px / l; ny = py / l; nz = pz / l; }
			}
		}
#endif
