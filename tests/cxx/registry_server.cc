// Every registered "hip" kernel of the C++ mirror as a single call through kman->setup<T> / kman->run<T> with the
// mirror's own types (stencil_op<sten>, grid_func, relax_stencil, prolong_op, restrict_op), driven by
// tests/test_cxx_registry.py so that the kernel suites of tests/cases.py run through the registry.
//
// One request per line on stdin, one answer per line on stdout ("ok", or "error <why>").  Arrays travel as files of
// raw doubles in the kernels' own layout; extents are interior extents.  Requests:
//   manager <dim> <per_mask> [<plane-config key>=<value> ...]      new kernel_params, new manager
//   setup_recip <nst> <n..> <so> <sor>                             point_relax set-up; writes sor
//   relax <nst> <n..> <updown> <so> <qf> <q> <sor>                 writes q
//   setup_lines <x|y> <nst> <n..> <so> <sor>                       2D; writes sor
//   relax_lines <x|y> <nst> <n..> <updown> <so> <qf> <q> <sor>     2D; writes q
//   residual <nst> <n..> <so> <qf> <q> <res>                       writes res
//   setup_interp <nst> <n..> <nc..> <so> <ci>                      writes ci
//   galerkin <nst> <n..> <nc..> <so> <soc> <ci>                    writes soc
//   restrict <n..> <nc..> <q> <qc> <ci>                            writes qc and q
//   interp_add <nst> <n..> <nc..> <q> <qc> <res> <so> <ci>         writes q and res
//   setup_cg <nst> <n..> <n1> <n2> <so> <abd>                      writes abd
//   solve_cg <n..> <n1> <n2> <q> <qf> <abd>                        writes q
//   planes <xy|xz|yz> <nst> <n..> <updown> <nsetup> <so> <x> <b>   3D; set-up nsetup times, one run; writes x
//   quit
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <cedar/2d/solver.h>
#include <cedar/3d/solver.h>

using namespace cedar;

struct bad_request { std::string why; };

template <class A> static void load(const std::string & path, A & a)
{
	std::ifstream f(path, std::ios::binary | std::ios::ate);
	if (!f || static_cast<std::size_t>(f.tellg()) != a.size() * sizeof(real_t))
		throw bad_request{path + " is missing or does not hold " + std::to_string(a.size()) + " doubles"};
	f.seekg(0);
	f.read(reinterpret_cast<char *>(a.data()), static_cast<std::streamsize>(a.size() * sizeof(real_t)));
}
template <class A> static void store(const std::string & path, const A & a)
{
	std::ofstream f(path, std::ios::binary);
	f.write(reinterpret_cast<const char *>(a.data()), static_cast<std::streamsize>(a.size() * sizeof(real_t)));
}

// the words of one request, taken in order
struct words {
	std::vector<std::string> w;
	std::size_t at = 0;
	const std::string & next()
	{
		if (at >= w.size()) throw bad_request{"too few words"};
		return w[at++];
	}
	int num()
	{
		const std::string & s = next();
		char * end = nullptr;
		const long v = std::strtol(s.c_str(), &end, 10);
		if (end == s.c_str() || *end || v < 0 || v > (1 << 24)) throw bad_request{"not a count: " + s};
		return (int)v;
	}
};

template <int dim> struct tr;
template <> struct tr<2> {
	using ST = cdr2::stypes;
	using comp = cdr2::five_pt;
	using full = cdr2::nine_pt;
	using gf = cdr2::grid_func;
	using rs = cdr2::relax_stencil;
	using po = cdr2::prolong_op;
	using ro = cdr2::restrict_op;
	template <class sten> using op = cdr2::stencil_op<sten>;
	static const int ncomp = 3, nfull = 5;
	template <class T> static T make(const len_t * n) { return T(n[0], n[1]); }
	static gf matrix(len_t n1, len_t n2) { return gf(n1, n2, 0); }
	static void fine(po & P, op<comp> & A) { P.fine_op_five = &A; P.fine_is_five = true; }
	static void fine(po & P, op<full> & A) { P.fine_op_nine = &A; P.fine_is_five = false; }
};
template <> struct tr<3> {
	using ST = cdr3::stypes;
	using comp = cdr3::seven_pt;
	using full = cdr3::xxvii_pt;
	using gf = cdr3::grid_func;
	using rs = cdr3::relax_stencil;
	using po = cdr3::prolong_op;
	using ro = cdr3::restrict_op;
	template <class sten> using op = cdr3::stencil_op<sten>;
	static const int ncomp = 4, nfull = 14;
	template <class T> static T make(const len_t * n) { return T(n[0], n[1], n[2]); }
	static gf matrix(len_t n1, len_t n2) { return gf::matrix(n1, n2); }
	static void fine(po & P, op<comp> & A) { P.fine_op_seven = &A; P.fine_is_seven = true; }
	static void fine(po & P, op<full> & A) { P.fine_op_xxvii = &A; P.fine_is_seven = false; }
};

static std::shared_ptr<kernel_manager> km;

template <int dim> static void extents(words & w, len_t * n) { for (int d = 0; d < dim; d++) n[d] = w.num(); }
static cycle::Dir updown(words & w) { return w.num() ? cycle::Dir::UP : cycle::Dir::DOWN; }

// requests that take the operator: sten is its stencil
template <int dim, class sten> static void with_op(const std::string & what, words & w)
{
	using T = tr<dim>;
	using ST = typename T::ST;
	using op = typename T::template op<sten>;
	using fop = typename T::template op<typename T::full>;
	using gf = typename T::gf;
	len_t n[3] = {1, 1, 1}, nc[3] = {1, 1, 1};
	if (what == "setup_recip") {
		extents<dim>(w, n);
		op so = T::template make<op>(n);
		typename T::rs sor = T::template make<typename T::rs>(n);
		load(w.next(), so);
		const std::string fsor = w.next();
		load(fsor, sor);
		km->setup<kernels::point_relax<ST>>(so, sor);
		store(fsor, sor);
	} else if (what == "relax") {
		extents<dim>(w, n);
		const cycle::Dir dir = updown(w);
		op so = T::template make<op>(n);
		gf qf = T::template make<gf>(n), q = T::template make<gf>(n);
		typename T::rs sor = T::template make<typename T::rs>(n);
		load(w.next(), so);
		load(w.next(), qf);
		const std::string fq = w.next();
		load(fq, q);
		load(w.next(), sor);
		km->run<kernels::point_relax<ST>>(so, q, qf, sor, dir);
		store(fq, q);
	} else if (what == "residual") {
		extents<dim>(w, n);
		op so = T::template make<op>(n);
		gf qf = T::template make<gf>(n), q = T::template make<gf>(n), res = T::template make<gf>(n);
		load(w.next(), so);
		load(w.next(), qf);
		load(w.next(), q);
		const std::string fres = w.next();
		load(fres, res);
		km->run<kernels::residual<ST>>(so, q, qf, res);
		store(fres, res);
	} else if (what == "setup_interp") {
		extents<dim>(w, n);
		extents<dim>(w, nc);
		op so = T::template make<op>(n);
		fop cop = T::template make<fop>(nc);
		typename T::po P = T::template make<typename T::po>(nc);
		load(w.next(), so);
		const std::string fci = w.next();
		load(fci, P);
		km->run<kernels::setup_interp<ST>>(so, cop, P);
		store(fci, P);
	} else if (what == "galerkin") {
		extents<dim>(w, n);
		extents<dim>(w, nc);
		op so = T::template make<op>(n);
		fop cop = T::template make<fop>(nc);
		typename T::po P = T::template make<typename T::po>(nc);
		load(w.next(), so);
		const std::string fsoc = w.next();
		load(fsoc, cop);
		load(w.next(), P);
		T::fine(P, so);
		km->run<kernels::coarsen_op<ST>>(P, so, cop);
		store(fsoc, cop);
	} else if (what == "interp_add") {
		extents<dim>(w, n);
		extents<dim>(w, nc);
		op so = T::template make<op>(n);
		gf q = T::template make<gf>(n), res = T::template make<gf>(n), qc = T::template make<gf>(nc);
		typename T::po P = T::template make<typename T::po>(nc);
		const std::string fq = w.next();
		load(fq, q);
		load(w.next(), qc);
		const std::string fres = w.next();
		load(fres, res);
		load(w.next(), so);
		load(w.next(), P);
		T::fine(P, so); // what setup_interp leaves in the prolongation: interp_add divides by the fine diagonal
		km->run<kernels::interp_add<ST>>(P, qc, res, q);
		store(fq, q);
		store(fres, res);
	} else if (what == "setup_cg") {
		extents<dim>(w, n);
		const len_t n1 = w.num(), n2 = w.num();
		op so = T::template make<op>(n);
		gf abd = T::matrix(n1, n2);
		load(w.next(), so);
		const std::string fabd = w.next();
		load(fabd, abd);
		km->setup<kernels::solve_cg<ST>>(so, abd);
		store(fabd, abd);
	} else if (what == "setup_lines" || what == "relax_lines") {
		if constexpr (dim == 2) {
			const bool isx = w.w[1] == "x"; // the direction came before the stencil
			extents<dim>(w, n);
			op so = T::template make<op>(n);
			typename T::rs sor = T::template make<typename T::rs>(n);
			using lx = kernels::line_relax<ST, relax_dir::x>;
			using ly = kernels::line_relax<ST, relax_dir::y>;
			if (what == "setup_lines") {
				load(w.next(), so);
				const std::string fsor = w.next();
				load(fsor, sor);
				if (isx) km->setup<lx>(so, sor);
				else km->setup<ly>(so, sor);
				store(fsor, sor);
			} else {
				const cycle::Dir dir = updown(w);
				gf qf = T::template make<gf>(n), q = T::template make<gf>(n), res = T::template make<gf>(n);
				load(w.next(), so);
				load(w.next(), qf);
				const std::string fq = w.next();
				load(fq, q);
				load(w.next(), sor);
				if (isx) km->run<lx>(so, q, qf, sor, res, dir);
				else km->run<ly>(so, q, qf, sor, res, dir);
				store(fq, q);
			}
		} else throw bad_request{"line relaxation is a 2D kernel"};
	} else if (what == "planes") {
		if constexpr (dim == 3) {
			const std::string d = w.w[1];
			extents<dim>(w, n);
			const cycle::Dir dir = updown(w);
			const int nsetup = w.num();
			op so = T::template make<op>(n);
			gf x = T::template make<gf>(n), b = T::template make<gf>(n);
			load(w.next(), so);
			const std::string fx = w.next();
			load(fx, x);
			load(w.next(), b);
			auto go = [&](auto tag) {
				using pr = kernels::plane_relax<ST, decltype(tag)::value>;
				for (int i = 0; i < nsetup; i++) km->setup<pr>(so);
				km->run<pr>(so, x, b, dir);
			};
			if (d == "xy") go(std::integral_constant<relax_dir, relax_dir::xy>());
			else if (d == "xz") go(std::integral_constant<relax_dir, relax_dir::xz>());
			else if (d == "yz") go(std::integral_constant<relax_dir, relax_dir::yz>());
			else throw bad_request{"no plane direction " + d};
			store(fx, x);
		} else throw bad_request{"plane relaxation is a 3D kernel"};
	} else throw bad_request{"no request " + what};
}

template <int dim> static void request(const std::string & what, words & w)
{
	using T = tr<dim>;
	using ST = typename T::ST;
	using gf = typename T::gf;
	len_t n[3] = {1, 1, 1}, nc[3] = {1, 1, 1};
	if (what == "restrict") {
		extents<dim>(w, n);
		extents<dim>(w, nc);
		gf q = T::template make<gf>(n), qc = T::template make<gf>(nc);
		typename T::po P = T::template make<typename T::po>(nc);
		const std::string fq = w.next(), fqc = w.next();
		load(fq, q);
		load(fqc, qc);
		load(w.next(), P);
		typename T::ro R(&P);
		km->run<kernels::restriction<ST>>(R, q, qc);
		store(fqc, qc);
		store(fq, q);
	} else if (what == "solve_cg") {
		extents<dim>(w, n);
		const len_t n1 = w.num(), n2 = w.num();
		gf q = T::template make<gf>(n), qf = T::template make<gf>(n), abd = T::matrix(n1, n2);
		const std::string fq = w.next();
		load(fq, q);
		load(w.next(), qf);
		load(w.next(), abd);
		std::vector<real_t> bbd(n2, 0.0);
		km->run<kernels::solve_cg<ST>>(q, qf, abd, bbd.data());
		store(fq, q);
	} else {
		if (what == "setup_lines" || what == "relax_lines" || what == "planes") w.next(); // the direction
		const int nst = w.num();
		if (nst == T::ncomp) with_op<dim, typename T::comp>(what, w);
		else if (nst == T::nfull) with_op<dim, typename T::full>(what, w);
		else throw bad_request{"no stencil of " + std::to_string(nst) + " entries in " + std::to_string(dim) + "D"};
	}
}

int main()
{
	log::status.on = false;
	int dim = 0;
	std::string line;
	while (std::getline(std::cin, line)) {
		words w;
		std::istringstream is(line);
		for (std::string s; is >> s;) w.w.push_back(s);
		if (w.w.empty()) continue;
		try {
			const std::string what = w.next();
			if (what == "quit") break;
			if (what == "manager") {
				const int d = w.num(), mask = w.num();
				if (d != 2 && d != 3) throw bad_request{"dim must be 2 or 3"};
				config c{config::empty_tag()};
				for (int i = 0; i < 3; i++) c.set("grid.periodic." + std::to_string(i), (mask >> i) & 1);
				while (w.at < w.w.size()) {
					const std::string & kv = w.next();
					const auto eq = kv.find('=');
					if (eq == std::string::npos) throw bad_request{"not key=value: " + kv};
					c.set("plane-config." + kv.substr(0, eq), kv.substr(eq + 1));
				}
				km = d == 2 ? cdr2::build_kernel_manager(c) : cdr3::build_kernel_manager(c);
				dim = d;
			} else if (dim == 2) request<2>(what, w);
			else if (dim == 3) request<3>(what, w);
			else throw bad_request{"no manager yet"};
			std::cout << "ok" << std::endl;
		} catch (const bad_request & e) {
			std::cout << "error " << e.why << std::endl;
		}
	}
	return 0;
}
