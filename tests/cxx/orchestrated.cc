// The orchestrated driver of the C++ mirror (include/cedar/multilevel.h: setup_impl, ncycle_helper, fmg_cycle, the
// host-side solve loop) on the GPU, one process per case, driven by tests/test_cxx_registry.py.
//
//   orchestrated <dir>
//
// <dir>/config.json is the solver's configuration plus a "test" block {mode, dim, n: [nx, ny, nz], nst, vcycle};
// <dir>/so.bin and b.bin (and x0.bin for vcycle) hold the operator, the right-hand side and a first guess, written
// by the test from tests/problems.py.  Modes:
//   case    1. resident solve; 2. on the same solver, levels untouched, force_orchestrated and solve, then every
//           level's A / P / SOR as the manager set them up (mgr_*), optionally one vcycle(x, b) off the resident path;
//           3. a second solver: resident solve, then the downloaded levels (dl_*)
//   count   every abstract kernel class replaced by a counting wrapper registered as "user" and selected before the
//           first solve; a second, all-"hip" orchestrated solve for the bit-for-bit comparison
//   defect  resident solve, a read of levels.get(1).A, then force_orchestrated and solve
// One line of JSON on stdout, arrays as raw doubles under <dir>.
#include <cstdio>
#include <fstream>
#include <map>
#include <string>
#include <cedar/2d/solver.h>
#include <cedar/3d/solver.h>

using namespace cedar;

template <class A> static void dump(const std::string & path, const A & a)
{
	std::ofstream f(path, std::ios::binary);
	f.write(reinterpret_cast<const char *>(a.data()), static_cast<std::streamsize>(a.size() * sizeof(real_t)));
}

template <class A> static bool load(const std::string & path, A & a)
{
	std::ifstream f(path, std::ios::binary | std::ios::ate);
	if (!f || static_cast<std::size_t>(f.tellg()) != a.size() * sizeof(real_t)) {
		std::fprintf(stderr, "orchestrated: %s is missing or does not hold %zu doubles\n", path.c_str(), a.size());
		return false;
	}
	f.seekg(0);
	f.read(reinterpret_cast<char *>(a.data()), static_cast<std::streamsize>(a.size() * sizeof(real_t)));
	return true;
}

template <int dim, class T> static T make(len_t nx, len_t ny, len_t nz)
{
	if constexpr (dim == 2) return T(nx, ny);
	else return T(nx, ny, nz);
}

static void print_hist(const char * key, const std::vector<real_t> & h)
{
	std::printf("\"%s\": [", key);
	for (std::size_t i = 0; i < h.size(); i++) std::printf("%s%.17g", i ? ", " : "", h[i]);
	std::printf("], ");
}

// ---- counting wrappers: the reference's abstract classes, arithmetic left to the library's bindings
struct tally_t { int setup = 0, run = 0; };
static std::map<std::string, tally_t> tally;

template <class ST> struct kt {
	using opc = typename ST::template stencil_op<typename ST::comp_sten>;
	using opf = typename ST::template stencil_op<typename ST::full_sten>;
	using gf = typename ST::grid_func;
	using rs = typename ST::relax_stencil;
	using po = typename ST::prolong_op;
	using ro = typename ST::restrict_op;
	using params = std::shared_ptr<kernel_params>;
};

template <class ST, class impl> struct c_residual : kernels::residual<ST> {
	using t = kt<ST>;
	explicit c_residual(typename t::params p) { inner.add_params(p); }
	void run(const typename t::opc & so, const typename t::gf & x, const typename t::gf & b, typename t::gf & r) override { tally["residual"].run++; inner.run(so, x, b, r); }
	void run(const typename t::opf & so, const typename t::gf & x, const typename t::gf & b, typename t::gf & r) override { tally["residual"].run++; inner.run(so, x, b, r); }
	impl inner;
};
template <class ST, class impl> struct c_restriction : kernels::restriction<ST> {
	using t = kt<ST>;
	explicit c_restriction(typename t::params p) { inner.add_params(p); }
	void run(const typename t::ro & R, const typename t::gf & x, typename t::gf & y) override { tally["restriction"].run++; inner.run(R, x, y); }
	impl inner;
};
template <class ST, class impl> struct c_interp_add : kernels::interp_add<ST> {
	using t = kt<ST>;
	explicit c_interp_add(typename t::params p) { inner.add_params(p); }
	void run(const typename t::po & P, const typename t::gf & c, const typename t::gf & r, typename t::gf & f) override { tally["interp_add"].run++; inner.run(P, c, r, f); }
	impl inner;
};
template <class ST, class impl> struct c_setup_interp : kernels::setup_interp<ST> {
	using t = kt<ST>;
	explicit c_setup_interp(typename t::params p) { inner.add_params(p); }
	void run(const typename t::opc & fop, const typename t::opf & cop, typename t::po & P) override { tally["setup_interp"].run++; inner.run(fop, cop, P); }
	void run(const typename t::opf & fop, const typename t::opf & cop, typename t::po & P) override { tally["setup_interp"].run++; inner.run(fop, cop, P); }
	impl inner;
};
template <class ST, class impl> struct c_coarsen_op : kernels::coarsen_op<ST> {
	using t = kt<ST>;
	explicit c_coarsen_op(typename t::params p) { inner.add_params(p); }
	void run(const typename t::po & P, const typename t::opc & fop, typename t::opf & cop) override { tally["coarsen_op"].run++; inner.run(P, fop, cop); }
	void run(const typename t::po & P, const typename t::opf & fop, typename t::opf & cop) override { tally["coarsen_op"].run++; inner.run(P, fop, cop); }
	impl inner;
};
template <class ST, class impl> struct c_solve_cg : kernels::solve_cg<ST> {
	using t = kt<ST>;
	explicit c_solve_cg(typename t::params p) { inner.add_params(p); }
	void setup(const typename t::opc & so, typename t::gf & ABD) override { tally["solve_cg"].setup++; inner.setup(so, ABD); }
	void setup(const typename t::opf & so, typename t::gf & ABD) override { tally["solve_cg"].setup++; inner.setup(so, ABD); }
	void run(typename t::gf & x, const typename t::gf & b, const typename t::gf & ABD, real_t * bbd) override { tally["solve_cg"].run++; inner.run(x, b, ABD, bbd); }
	impl inner;
};
template <class ST, relax_dir d, class impl> struct c_lines : kernels::line_relax<ST, d> {
	using t = kt<ST>;
	explicit c_lines(typename t::params p) { inner.add_params(p); }
	static const char * key() { return d == relax_dir::x ? "line_relax_x" : "line_relax_y"; }
	void setup(const typename t::opc & so, typename t::rs & sor) override { tally[key()].setup++; inner.setup(so, sor); }
	void setup(const typename t::opf & so, typename t::rs & sor) override { tally[key()].setup++; inner.setup(so, sor); }
	void run(const typename t::opc & so, typename t::gf & x, const typename t::gf & b, const typename t::rs & sor, typename t::gf & res, cycle::Dir dir) override
	{ tally[key()].run++; inner.run(so, x, b, sor, res, dir); }
	void run(const typename t::opf & so, typename t::gf & x, const typename t::gf & b, const typename t::rs & sor, typename t::gf & res, cycle::Dir dir) override
	{ tally[key()].run++; inner.run(so, x, b, sor, res, dir); }
	impl inner;
};
template <class ST, relax_dir d, class impl> struct c_planes : kernels::plane_relax<ST, d> {
	using t = kt<ST>;
	explicit c_planes(typename t::params p) { inner.add_params(p); }
	void setup(const typename t::opc & so) override { tally["plane_relax_xy"].setup++; inner.setup(so); }
	void setup(const typename t::opf & so) override { tally["plane_relax_xy"].setup++; inner.setup(so); }
	void run(const typename t::opc & so, typename t::gf & x, const typename t::gf & b, cycle::Dir dir) override { tally["plane_relax_xy"].run++; inner.run(so, x, b, dir); }
	void run(const typename t::opf & so, typename t::gf & x, const typename t::gf & b, cycle::Dir dir) override { tally["plane_relax_xy"].run++; inner.run(so, x, b, dir); }
	impl inner;
};

// the kernels both dimensions share; NS is the namespace-like struct of the bindings
template <class ST, class B> static void select_counting(std::shared_ptr<kernel_manager> km)
{
	auto p = km->get_params();
	km->add<kernels::residual<ST>, c_residual<ST, typename B::residual>>("user", p);
	km->add<kernels::restriction<ST>, c_restriction<ST, typename B::restriction>>("user", p);
	km->add<kernels::interp_add<ST>, c_interp_add<ST, typename B::interp_add>>("user", p);
	km->add<kernels::setup_interp<ST>, c_setup_interp<ST, typename B::setup_interp>>("user", p);
	km->add<kernels::coarsen_op<ST>, c_coarsen_op<ST, typename B::coarsen_op>>("user", p);
	km->add<kernels::solve_cg<ST>, c_solve_cg<ST, typename B::solve_cg>>("user", p);
	km->set<kernels::residual<ST>>("user");
	km->set<kernels::restriction<ST>>("user");
	km->set<kernels::interp_add<ST>>("user");
	km->set<kernels::setup_interp<ST>>("user");
	km->set<kernels::coarsen_op<ST>>("user");
	km->set<kernels::solve_cg<ST>>("user");
}
struct bind2 {
	using residual = cdr2::residual_f90; using restriction = cdr2::restrict_f90; using interp_add = cdr2::interp_f90;
	using setup_interp = cdr2::setup_interp_f90; using coarsen_op = cdr2::galerkin; using solve_cg = cdr2::solve_cg_f90;
};
struct bind3 {
	using residual = cdr3::residual_f90; using restriction = cdr3::restrict_f90; using interp_add = cdr3::interp_f90;
	using setup_interp = cdr3::setup_interp_f90; using coarsen_op = cdr3::galerkin; using solve_cg = cdr3::solve_cg_f90;
};
static void select_counting_dim(std::shared_ptr<kernel_manager> km, std::integral_constant<int, 2>)
{
	using ST = cdr2::stypes;
	select_counting<ST, bind2>(km);
	auto p = km->get_params();
	km->add<kernels::line_relax<ST, relax_dir::x>, c_lines<ST, relax_dir::x, cdr2::lines<relax_dir::x>>>("user", p);
	km->add<kernels::line_relax<ST, relax_dir::y>, c_lines<ST, relax_dir::y, cdr2::lines<relax_dir::y>>>("user", p);
	km->set<kernels::line_relax<ST, relax_dir::x>>("user");
	km->set<kernels::line_relax<ST, relax_dir::y>>("user");
}
static void select_counting_dim(std::shared_ptr<kernel_manager> km, std::integral_constant<int, 3>)
{
	using ST = cdr3::stypes;
	select_counting<ST, bind3>(km);
	km->add<kernels::plane_relax<ST, relax_dir::xy>, c_planes<ST, relax_dir::xy, cdr3::planes<relax_dir::xy>>>("user", km->get_params());
	km->set<kernels::plane_relax<ST, relax_dir::xy>>("user");
}

template <class L> static void dump_level(const std::string & pre, L & lev, bool coarse, int nsor)
{
	if (coarse) {
		dump(pre + "_A.bin", lev.A);
		dump(pre + "_P.bin", lev.P);
	}
	for (int s = 0; s < nsor; s++) dump(pre + "_SOR" + std::to_string(s) + ".bin", lev.SOR[s]);
}

template <class S, class fsten> static void dump_levels(const std::string & out, const char * tag, S & s, int nsor)
{
	const std::size_t nlev = s.nlevels();
	dump_level(out + "/" + tag + "_L0", s.levels.template get<fsten>(0), false, nsor);
	for (std::size_t l = 1; l < nlev; l++) dump_level(out + "/" + tag + "_L" + std::to_string(l), s.levels.get(l), true, nsor);
}

template <int dim, class S, class fsten, class OP, class GF>
static int drive(const std::string & out, std::shared_ptr<config> conf, len_t nx, len_t ny, len_t nz)
{
	const std::string mode = conf->get<std::string>("test.mode", "case");
	OP so = make<dim, OP>(nx, ny, nz);
	GF b = make<dim, GF>(nx, ny, nz);
	if (!load(out + "/so.bin", so) || !load(out + "/b.bin", b)) return 2;
	const int nsor = dim == 2 ? 2 : 1;
	std::printf("{\"mode\": \"%s\", ", mode.c_str());
	if (mode == "case") {
		S s(so, conf);
		const bool res0 = s.resident();
		GF x = s.solve(b);
		print_hist("hist_resident", s.history);
		dump(out + "/res_x.bin", x);
		s.force_orchestrated = true;
		GF xo = s.solve(b);
		print_hist("hist_orchestrated", s.history);
		dump(out + "/orc_x.bin", xo);
		dump_levels<S, fsten>(out, "mgr", s, nsor);
		if (conf->get<int>("test.vcycle", 0)) {
			GF xv = make<dim, GF>(nx, ny, nz);
			if (!load(out + "/x0.bin", xv)) return 2;
			s.vcycle(xv, b);
			dump(out + "/vc_x.bin", xv);
		}
		S s2(so, conf);
		GF x2 = s2.solve(b);
		print_hist("hist_second", s2.history);
		dump_levels<S, fsten>(out, "dl", s2, nsor);
		std::printf("\"resident_before\": %d, \"nlevels\": %zu}\n", (int)res0, s.nlevels());
	} else if (mode == "count") {
		S s(so, conf);
		select_counting_dim(s.get_kernels(), std::integral_constant<int, dim>());
		const bool res0 = s.resident();
		s.solve(b);
		print_hist("hist_user", s.history);
		S h(so, conf);
		h.force_orchestrated = true;
		h.solve(b);
		print_hist("hist_hip", h.history);
		std::printf("\"counts\": {");
		bool first = true;
		for (auto & kv : tally) {
			std::printf("%s\"%s\": [%d, %d]", first ? "" : ", ", kv.first.c_str(), kv.second.setup, kv.second.run);
			first = false;
		}
		std::printf("}, \"resident_before\": %d, \"nlevels\": %zu}\n", (int)res0, s.nlevels());
	} else if (mode == "defect") {
		S s(so, conf);
		s.solve(b);
		print_hist("hist_resident", s.history);
		auto & A1 = s.levels.get(1).A; // the download: host arrays exist, smoothers and coarse solver do not
		const real_t a1 = A1.data()[A1.size() / 2];
		s.force_orchestrated = true;
		GF xo = s.solve(b);
		print_hist("hist_orchestrated", s.history);
		dump(out + "/orc_x.bin", xo);
		std::printf("\"a1\": %.17g, \"nlevels\": %zu}\n", a1, s.nlevels());
	} else {
		std::fprintf(stderr, "orchestrated: unknown mode %s\n", mode.c_str());
		return 2;
	}
	return 0;
}

int main(int argc, char ** argv)
{
	const std::string out = argc > 1 ? argv[1] : ".";
	auto conf = std::make_shared<config>(out + "/config.json");
	log::status.on = false;
	const int dim = conf->get<int>("test.dim", 2), nst = conf->get<int>("test.nst", 0);
	auto n = conf->getvec<int>("test.n");
	if ((int)n.size() != dim) { std::fprintf(stderr, "orchestrated: test.n must hold %d extents\n", dim); return 2; }
	if (dim == 2 && nst == 3)
		return drive<2, cdr2::solver<cdr2::five_pt>, cdr2::five_pt, cdr2::stencil_op<cdr2::five_pt>, cdr2::grid_func>(out, conf, n[0], n[1], 1);
	if (dim == 2 && nst == 5)
		return drive<2, cdr2::solver<cdr2::nine_pt>, cdr2::nine_pt, cdr2::stencil_op<cdr2::nine_pt>, cdr2::grid_func>(out, conf, n[0], n[1], 1);
	if (dim == 3 && nst == 4)
		return drive<3, cdr3::solver<cdr3::seven_pt>, cdr3::seven_pt, cdr3::stencil_op<cdr3::seven_pt>, cdr3::grid_func>(out, conf, n[0], n[1], n[2]);
	if (dim == 3 && nst == 14)
		return drive<3, cdr3::solver<cdr3::xxvii_pt>, cdr3::xxvii_pt, cdr3::stencil_op<cdr3::xxvii_pt>, cdr3::grid_func>(out, conf, n[0], n[1], n[2]);
	std::fprintf(stderr, "orchestrated: no solver for dim %d with %d stencil entries\n", dim, nst);
	return 2;
}
